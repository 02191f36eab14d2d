"""CPU: the match mode of the PNG encoder as tests/png_match_oracle.py restates it (include/rcdm.h, "PNG, match mode") —
that its files decode, are never larger than the literal-only files of tests/png_oracle.py, are much smaller on flat frames,
that the parse follows the rules of the format, and that the committed goldens (tools/mint_png_match_golden.py) are its output."""
import io
import json
import os
import zlib

import numpy as np
import pytest

from tests import png_match_oracle as M
from tests import png_oracle as P

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LITERAL_256 = 28633                                       # the literal-only file of cartoon(256, 256, 0.0, 1)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _cases():
    mixed = P.cartoon(256, 85, 0.0, 4)
    mixed[128:] = noise(128, 85, 104)
    return {"1x1": noise(1, 1, 1), "3x5": noise(3, 5, 2), "black": np.zeros((64, 64, 3), dtype=np.uint8),
            "w1": P.cartoon(40, 1, 0.0, 5), "w2": P.cartoon(40, 2, 0.0, 5), "w3": P.cartoon(40, 3, 0.0, 5),
            "flat105": P.cartoon(105, 107, 0.0, 3), "noisy105": P.cartoon(105, 107, 2.0, 3), "loud105": P.cartoon(105, 107, 40.0, 24),
            "mixed": mixed, "2x8192": P.cartoon(2, 8192, 0.0, 6), "33x31": P.cartoon(33, 31, 0.0, 7)}


CASES = _cases()


@pytest.fixture(scope="module")
def encoded():
    """name -> the match-mode file under the adaptive filter, computed once."""
    return {name: M.encode(img) for name, img in CASES.items()}


def check_decodes(data, img, filt):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)
    chunks = P.parse_chunks(data)
    for kind, _, stored, real in chunks:
        assert stored == real, f"CRC of a {kind!r} chunk"
    stream, _ = P.filter_stream(img, filt)
    assert zlib.decompress(b"".join(body for kind, body, _, _ in chunks if kind == b"IDAT")) == stream.tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_decodes(encoded, name):
    check_decodes(encoded[name], CASES[name], -1)
    assert len(encoded[name]) == M.png_size(CASES[name])


@pytest.mark.parametrize("name", list(CASES))
def test_never_larger(encoded, name):
    """Every case under every filter mode: adaptive and each fixed filter 0..4."""
    img = CASES[name]
    assert len(encoded[name]) <= len(P.encode(img))
    for f in range(5):
        data = M.encode(img, f)
        assert len(data) <= len(P.encode(img, f)), f
        check_decodes(data, img, f)


def test_all_blocks_fall_back_gives_the_literal_file():
    img = CASES["loud105"]
    stream, _ = P.filter_stream(img)
    for b0 in range(0, len(stream), P.BLOCK):
        _, mbits, lbits = M.block_forms(stream, b0, min(b0 + P.BLOCK, len(stream)), 1 + 3 * 107)
        assert mbits >= lbits, f"the block at {b0} would take the match form ({mbits} < {lbits}): not the image this test needs"
    assert M.encode(img) == P.encode(img)


def test_smaller_where_it_should_be():
    img = P.cartoon(256, 256, 0.0, 1)
    assert len(P.encode(img)) == LITERAL_256
    size = len(M.encode(img))
    raw = P.filter_stream(img)[0].tobytes()
    z1, z6 = len(zlib.compress(raw, 1)), len(zlib.compress(raw, 6))
    print(f"cartoon(256, 256, 0, 1): match mode {size} B = {size / LITERAL_256:.3f} x literal-only, {size / z1:.3f} x zlib level 1 "
          f"({z1} B), {size / z6:.3f} x zlib level 6 ({z6} B)")
    assert size <= 0.5 * LITERAL_256


def tokens(stream, b0=0, b1=None, row=None):
    return M.parse_block(np.asarray(stream, dtype=np.uint8), b0, len(stream) if b1 is None else b1, row)


@pytest.mark.parametrize("r", [0, 1, 2, 3, 4, 5])
def test_parse_run_longer_than_258(r):
    got = tokens([7] * (1 + 258 + r))
    want = [(0, 1, 0), (1, 258, 1)]
    want += [(259 + k, 1, 0) for k in range(r)] if r < 4 else [(259, r, 1)]
    assert got == want


def test_parse_run_stops_at_the_cut():
    s = [9, 4] + [5] * 300
    assert tokens(s, 0, 102) == [(0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 99, 1)]
    assert tokens(s, 102, 202) == [(102, 100, 1)]         # and the next block starts with a match into the previous one
    assert tokens(s, 0, 5)[-3:] == [(2, 1, 0), (3, 1, 0), (4, 1, 0)]   # 2 bytes left of the block: no usable match


def test_parse_source_only_in_the_previous_block():
    rng = np.random.RandomState(3)
    row = 40
    a = rng.randint(1, 255, size=row).astype(np.uint8)
    b = rng.randint(1, 255, size=row).astype(np.uint8)
    s = np.concatenate([a, b, a])                          # the third row repeats the first: distance 2 S only
    got = tokens(s, 2 * row, 3 * row, row)
    assert got == [(2 * row, row, 2 * row)]
    assert tokens(s, 2 * row, 3 * row, None) == [(2 * row + k, 1, 0) for k in range(row)]


def test_parse_distances_stay_inside_the_stream_and_the_window():
    for name in ("flat105", "mixed", "2x8192", "w1", "w2", "w3"):
        img = CASES[name]
        stream, _ = P.filter_stream(img)
        row = 1 + 3 * img.shape[1]
        for b0 in range(0, len(stream), P.BLOCK):
            b1 = min(b0 + P.BLOCK, len(stream))
            toks = M.parse_block(stream, b0, b1, row)
            assert toks[0][0] == b0 and sum(n for _, n, _ in toks) == b1 - b0
            for pos, n, d in toks:
                if d:
                    assert 1 <= d <= min(pos, M.WINDOW) and d in M.candidates(row) and M.MIN_MATCH <= n <= M.MAX_MATCH and pos + n <= b1
                    assert np.array_equal(stream[pos:pos + n], stream[pos - d:pos - d + n])
                    assert (n, d) == M.match_at(stream, pos, b1, row)
                else:
                    assert n == 1 and M.match_at(stream, pos, b1, row)[0] < M.MIN_MATCH


def test_parse_ties_go_to_the_earlier_candidate():
    s = [3] * 40                                           # every small distance gives the same run
    assert tokens(s)[:2] == [(0, 1, 0), (1, 39, 1)]
    s = [1, 2, 3] * 20                                     # distances 3, 6, 9, 12 tie from position 12 on; 3 is the earliest
    assert tokens(s)[3] == (3, 57, 3)
    row = 10                                               # S - 3 = 7 and 2 S = 20 ... a pattern of period 10: S before 2 S
    s = list(np.random.RandomState(5).randint(1, 255, size=10)) * 4
    got = tokens(s, 20, 40, row)
    assert got == [(20, 20, 10)]


def run_length(stream, pos, b1, d):
    k = 0
    while k < min(M.MAX_MATCH, b1 - pos) and stream[pos + k] == stream[pos + k - d]:
        k += 1
    return k


@pytest.mark.parametrize("w", [1, 2, 3])
def test_parse_duplicate_candidates(w):
    row = 1 + 3 * w
    cand = M.candidates(row)
    assert cand[:7] == [1, 2, 3, 4, 6, 9, 12] and cand[7:] == [row - 3, row, row + 3, 2 * row]
    assert (len(set(cand)) < len(cand)) == (w < 3)          # S - 3 repeats 1 or 4; at w = 3 the list is 7, 10, 13, 20
    stream, _ = P.filter_stream(CASES[f"w{w}"])
    matches = 0
    for pos, n, d in M.parse_block(stream, 0, len(stream), row):
        runs = [(run_length(stream, pos, len(stream), c), c) for c in cand if 1 <= c <= pos]
        longest = max([r for r, _ in runs], default=0)
        if d:
            assert n == longest and d == next(c for r, c in runs if r == longest)   # the first in the list at that length
            matches += 1
        else:
            assert longest < M.MIN_MATCH
    assert matches > 0


def test_parse_wide_rows_drop_2s_and_keep_s_plus_3():
    w = 8192
    row = 1 + 3 * w
    assert 2 * row > M.WINDOW >= row + 3
    rng = np.random.RandomState(9)
    a = rng.randint(1, 255, size=row).astype(np.uint8)
    s = np.concatenate([a, np.zeros(3, dtype=np.uint8), a[:200]])   # a[:200] again at distance S + 3
    assert tokens(s, row + 3, len(s), row) == [(row + 3, 200, row + 3)]
    s2 = np.concatenate([a, rng.randint(1, 255, size=row).astype(np.uint8), a[:200]])   # ... at 2 S, which is dropped
    assert all(d == 0 for _, _, d in tokens(s2, 2 * row, len(s2), row))
    for pos in (0, 5, row + 7, 2 * row):
        assert M.match_at(s2, pos, len(s2), row)[1] <= min(pos, M.WINDOW)


def test_limiter_on_the_286_symbol_alphabet():
    counts = np.zeros(M.NLL, dtype=np.int64)
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    counts[[0, 7, 255, 256, 257, 264, 285] + list(range(100, 117))] = fib
    assert P.huffman_depths(counts).max() > 15
    lens, halvings = M.limited_lengths(counts)
    assert halvings >= 1 and lens.max() <= 15 and ((lens > 0) == (counts > 0)).all()
    assert P.kraft(lens)[0] == P.kraft(lens)[1]
    one = np.zeros(M.NDIST, dtype=np.int64)
    one[17] = 5
    assert M.limited_lengths(one)[0].tolist() == [1 if k == 17 else 0 for k in range(M.NDIST)]


def test_length_and_distance_symbols_follow_rfc1951():
    base_l = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra_l = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    for n in range(3, 259):
        k = max(i for i in range(29) if base_l[i] <= n)
        assert M.length_symbol(n) == (257 + k, extra_l[k], n - base_l[k]), n
    base_d = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577]
    for d in list(range(1, 2000)) + [24576, 24577, 24580, 32767, 32768]:
        k = max(i for i in range(30) if base_d[i] <= d)
        assert M.distance_symbol(d) == (k, max(0, k // 2 - 1), d - base_d[k]), d


GOLDENS = ["pngm_1x1", "pngm_3x5", "pngm_black", "pngm_w1", "pngm_w2", "pngm_w3", "pngm_105x107", "pngm_256x85", "pngm_300x85",
           "pngm_2x8192", "pngm_batch", "pngm_f0", "pngm_f1", "pngm_f2", "pngm_f3", "pngm_f4", "pngm_limiter"]


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_is_the_oracles_output(name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    filt = json.loads(str(g["meta"]))["filter"]
    ends = np.cumsum(g["sizes"])
    for img, size, end in zip(g["input"], g["sizes"], ends):
        data = g["files"][end - size:end].tobytes()
        assert data == M.encode(img, filt)
        check_decodes(data, img, filt)
        assert len(data) <= len(P.encode(img, filt))
