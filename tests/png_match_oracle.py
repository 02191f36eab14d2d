"""numpy / Python restatement of the PNG files rcdm_png_encode_match writes (include/rcdm.h, "PNG, match mode"), byte for byte.

Everything of tests/png_oracle.py holds (filters, the cut every 32768 filtered bytes, one IDAT per block, the empty stored
block behind each, zlib header, Adler-32, container) except what a block's dynamic-Huffman block holds:
  candidates  at stream position i of a block [b0, b1) of an image with filtered rows of S = 1 + 3 w bytes, the distances
              1, 2, 3, 4, 6, 9, 12, S - 3, S, S + 3, 2 S in this order; d is dropped if d < 1, d > 32768 or d > i
  length      of candidate d: the count of k >= 0 with s[i + k] == s[i + k - d], capped at 258 and at b1 - i (the source may
              lie in front of b0); the longest candidate wins, the earlier one on a tie; usable from 4
  parse       greedy from b0: a usable match emits (length, distance) and skips it, otherwise the literal
  match form  HLIT 286, HDIST 30, HCLEN 19, the fixed 4-bit code-length code: a header of 1338 bits; both codes by the
              two-queue construction with the (c + 1) >> 1 limiter, each on its own counts; ONE used distance -> length 1
  fallback    the block takes the match form only if its bits up to and including end-of-block are STRICTLY fewer than the
              literal form's (png_oracle.deflate_block); otherwise its bytes are the literal form's

`encode` packs the bits; `png_size` gives the same length from the parse and the code lengths alone."""
import struct
import zlib

import numpy as np

from tests.png_oracle import (ADAPTIVE, BLOCK, MAX_BITS, SIGNATURE, canonical_codes, chunk, code_lengths, filter_stream,
                              huffman_depths)
from tests import png_oracle as P

MIN_MATCH, MAX_MATCH, WINDOW = 4, 258, 32768
NLL, NDIST = 286, 30
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (NLL + NDIST) * 4   # 1338


def candidates(row):
    """The candidate distances in order; `row` is S = 1 + 3 w, None leaves the row-dependent ones out."""
    c = [1, 2, 3, 4, 6, 9, 12]
    if row is not None:
        c += [row - 3, row, row + 3, 2 * row]
    return c


def match_at(stream, i, b1, row=None):
    """-> (length, distance) of the position's match (0, 0 if no candidate is left); the length may be below MIN_MATCH."""
    best, dist = 0, 0
    cap = min(MAX_MATCH, b1 - i)
    for d in candidates(row):
        if d < 1 or d > WINDOW or d > i:
            continue
        k = 0
        while k < cap and stream[i + k] == stream[i + k - d]:
            k += 1
        if k > best:
            best, dist = k, d
    return best, dist


def _best(stream, b0, b1, row):
    """Vectorised match_at over [b0, b1): (length [b1 - b0], distance [b1 - b0])."""
    s = np.asarray(stream)
    n = b1 - b0
    pos = np.arange(b0, b1)
    best = np.zeros(n, dtype=np.int64)
    dist = np.zeros(n, dtype=np.int64)
    for d in candidates(row):
        if d < 1 or d > WINDOW:
            continue
        ok = pos >= d
        eq = np.zeros(n + 1, dtype=bool)                  # eq[n]: the cut ends every run
        eq[:n][ok] = s[pos[ok]] == s[pos[ok] - d]
        zeros = np.flatnonzero(~eq)
        run = zeros[np.searchsorted(zeros, np.arange(n))] - np.arange(n)
        run = np.minimum(run, MAX_MATCH)
        win = run > best
        best[win], dist[win] = run[win], d
    return best, dist


def parse_block(stream, b0, b1, row=None):
    """The greedy parse of block [b0, b1) -> [(pos, len, dist)]; a literal is (pos, 1, 0)."""
    best, dist = _best(stream, b0, b1, row)
    out, i = [], b0
    while i < b1:
        if best[i - b0] >= MIN_MATCH:
            out.append((i, int(best[i - b0]), int(dist[i - b0])))
            i += int(best[i - b0])
        else:
            out.append((i, 1, 0))
            i += 1
    return out


def length_symbol(n):
    """RFC 1951 3.2.5: match length 3..258 -> (symbol, extra bits, extra value)."""
    if n == 258:
        return 285, 0, 0
    v = n - 3
    if v < 8:
        return 257 + v, 0, 0
    eb = v.bit_length() - 3
    return 261 + 4 * eb + ((v >> eb) & 3), eb, v & ((1 << eb) - 1)


def distance_symbol(d):
    """RFC 1951 3.2.5: distance 1..32768 -> (symbol, extra bits, extra value)."""
    v = d - 1
    if v < 4:
        return v, 0, 0
    n = v.bit_length() - 1
    return 2 * n + ((v >> (n - 1)) & 1), n - 1, v & ((1 << (n - 1)) - 1)


def limited_lengths(counts):
    """counts int [n] -> (lengths int [n], halvings): the two-queue code, limited to 15 bits by halving; fewer than two used
    symbols: the one used symbol gets length 1."""
    counts = np.asarray(counts, dtype=np.int64)
    used = np.flatnonzero(counts)
    if len(used) < 2:
        lens = np.zeros(len(counts), dtype=np.int64)
        lens[used] = 1
        return lens, 0
    halvings = 0
    while True:
        lens = huffman_depths(counts)
        if lens.max() <= MAX_BITS:
            return lens, halvings
        counts = np.where(counts > 0, (counts + 1) >> 1, 0)
        halvings += 1


def match_counts(stream, parse):
    """-> (literal / length counts [286] with end-of-block = 1, distance counts [30], extra bits in total)."""
    ll = np.zeros(NLL, dtype=np.int64)
    dd = np.zeros(NDIST, dtype=np.int64)
    extra = 0
    for pos, n, d in parse:
        if d:
            ls, le, _ = length_symbol(n)
            ds, de, _ = distance_symbol(d)
            ll[ls] += 1
            dd[ds] += 1
            extra += le + de
        else:
            ll[stream[pos]] += 1
    ll[256] = 1
    return ll, dd, extra


def block_forms(stream, b0, b1, row):
    """-> (parse, match-form bits, literal-form bits), each count up to and including the end-of-block code."""
    s = np.asarray(stream)
    parse = parse_block(s, b0, b1, row)
    ll, dd, extra = match_counts(s, parse)
    ll_len, _ = limited_lengths(ll)
    d_len, _ = limited_lengths(dd)
    mbits = HEADER_BITS + int((ll * ll_len).sum()) + int((dd * d_len).sum()) + extra
    hist = np.bincount(s[b0:b1], minlength=256)
    lens, _ = code_lengths(hist)
    return parse, mbits, P.block_bits(hist, lens)


def _rev(code, n):
    return int(f"{int(code):0{n}b}"[::-1], 2) if n else 0


def match_block(stream, parse, final):
    """One block in match form -> the bytes of its dynamic block + the empty stored block."""
    s = np.asarray(stream)
    ll, dd, _ = match_counts(s, parse)
    ll_len, _ = limited_lengths(ll)
    d_len, _ = limited_lengths(dd)
    ll_code, d_code = canonical_codes(ll_len), canonical_codes(d_len)
    val, nb = [], []

    def put(v, n):
        if n:
            val.append(int(v))
            nb.append(int(n))
    put(0, 1)                                             # BFINAL
    put(2, 2)                                             # BTYPE: dynamic
    put(NLL - 257, 5)
    put(NDIST - 1, 5)
    put(15, 4)                                            # HCLEN 19
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        val.append(0 if sym >= 16 else 4)
        nb.append(3)
    for l in list(ll_len) + list(d_len):
        val.append(_rev(l, 4))
        nb.append(4)
    assert sum(nb) == HEADER_BITS
    for pos, n, d in parse:
        if d:
            ls, le, lv = length_symbol(n)
            ds, de, dv = distance_symbol(d)
            put(_rev(ll_code[ls], ll_len[ls]), ll_len[ls])
            put(lv, le)
            put(_rev(d_code[ds], d_len[ds]), d_len[ds])
            put(dv, de)
        else:
            b = s[pos]
            put(_rev(ll_code[b], ll_len[b]), ll_len[b])
    put(_rev(ll_code[256], ll_len[256]), ll_len[256])
    put(1 if final else 0, 3)                             # the empty stored block's header
    acc, n, out = 0, 0, bytearray()
    for v, k in zip(val, nb):
        acc |= v << n
        n += k
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
    if n:
        out.append(acc & 255)
    return bytes(out) + b"\x00\x00\xff\xff"


def encode_blocks(img, filt=ADAPTIVE):
    """-> (stream, [(body bytes of the block, took the match form)])."""
    img = np.asarray(img)
    h, w, _ = img.shape
    stream, _ = filter_stream(img, filt)
    raw = stream.tobytes()
    nblk = -(-len(raw) // BLOCK)
    out = []
    for k in range(nblk):
        b0, b1 = k * BLOCK, min((k + 1) * BLOCK, len(raw))
        parse, mbits, lbits = block_forms(stream, b0, b1, 1 + 3 * w)
        if mbits < lbits:
            out.append((match_block(stream, parse, k == nblk - 1), True))
        else:
            out.append((P.deflate_block(raw[b0:b1], k == nblk - 1), False))
    return stream, out


def encode(img, filt=ADAPTIVE):
    """uint8 (h, w, 3) -> the PNG file as bytes."""
    img = np.asarray(img)
    h, w, _ = img.shape
    stream, blocks = encode_blocks(img, filt)
    raw = stream.tobytes()
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    for k, (body, _) in enumerate(blocks):
        if k == 0:
            body = b"\x78\x01" + body
        if k == len(blocks) - 1:
            body += struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
        out.append(chunk(b"IDAT", body))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def block_choice(img, filt=ADAPTIVE):
    """-> [took the match form] per block."""
    img = np.asarray(img)
    stream, _ = filter_stream(img, filt)
    w = img.shape[1]
    return [m < l for _, m, l in (block_forms(stream, b0, min(b0 + BLOCK, len(stream)), 1 + 3 * w)
                                  for b0 in range(0, len(stream), BLOCK))]


def png_size(img, filt=ADAPTIVE):
    """len(encode(img, filt)) from the parse and the code lengths of the blocks, without packing a bit."""
    img = np.asarray(img)
    stream, _ = filter_stream(img, filt)
    w = img.shape[1]
    total = 8 + 25 + 12 + 2 + 4
    for b0 in range(0, len(stream), BLOCK):
        _, mbits, lbits = block_forms(stream, b0, min(b0 + BLOCK, len(stream)), 1 + 3 * w)
        total += 12 + (min(mbits, lbits) + 3 + 7) // 8 + 4
    return total
