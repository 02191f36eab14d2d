"""numpy / Python restatement of the PNG files rcdm_png_encode writes (include/rcdm.h, "PNG"), byte for byte.

  filter     per scanline, bpp = 3, the row above the first row is zeros; `adaptive` takes the filter with the smallest
             sum of min(v, 256 - v) over the row's filtered bytes, the lowest filter number on a tie
  blocks     the filtered stream (h * (1 + 3 w) bytes) cut every 32768 bytes; one dynamic-Huffman deflate block over the
             literals and end-of-block per cut (HLIT 257, HDIST 1 with length 0, HCLEN 19, code-length code: 4 bits for
             0..15), then an empty stored block (BFINAL only behind the last) that pads to a byte
  code       Huffman by the two-queue construction: leaves ascending by (count, symbol), internal nodes in creation order,
             the leaf queue wins a tie; end-of-block counts 1; deeper than 15 -> every non-zero count becomes
             (c + 1) >> 1 and the code is rebuilt; canonical codes (RFC 1951 3.2.2)
  container  signature, IHDR, one IDAT per deflate block (zlib header 78 01 in the first, Adler-32 in the last), IEND

`encode` packs the bits; `png_size` gives the same length from histograms and code lengths alone."""
import struct
import zlib

import numpy as np

BLOCK = 32768
ADAPTIVE = -1
MAX_BITS = 15
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4        # 1106: block header, counts, code-length code, 257 + 1 lengths
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_FILTERS = {"adaptive": ADAPTIVE, "none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4}


def filter_id(f):
    f = _FILTERS.get(f, f) if isinstance(f, str) else int(f)
    if f not in (-1, 0, 1, 2, 3, 4):
        raise ValueError(f"filter {f!r}")
    return f


def filter_stream(img, filt=ADAPTIVE):
    """img uint8 (h, w, 3) -> (stream uint8 [h * (1 + 3 w)], types int [h])."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w, _ = img.shape
    x = img.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255
    filt = filter_id(filt)
    if filt < 0:
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)
        types = cost.argmin(axis=0)                      # the first minimum: the lowest filter number
    else:
        types = np.full(h, filt, dtype=np.int64)
    rows = cand[types, np.arange(h)]
    stream = np.concatenate([types[:, None], rows], axis=1).astype(np.uint8).reshape(-1)
    return stream, types


def huffman_depths(counts):
    """Leaf depths of the two-queue Huffman tree over the symbols with a non-zero count (no depth limit)."""
    order = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (int(counts[s]), s))
    n = len(order)
    assert n >= 2
    w = [int(counts[s]) for s in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j, nxt = 0, n, n
    while nxt < 2 * n - 1:
        pick = []
        for _ in range(2):
            if i < n and (j >= nxt or w[i] <= w[j]):     # the leaf queue wins a tie
                pick.append(i)
                i += 1
            else:
                pick.append(j)
                j += 1
        w[nxt] = w[pick[0]] + w[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
        nxt += 1
    depth = [0] * (2 * n - 1)
    for k in range(2 * n - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    out = np.zeros(len(counts), dtype=np.int64)
    out[order] = depth[:n]
    return out


def code_lengths(hist):
    """hist int [256] of one block -> (lengths int [257], halvings): end-of-block counts 1, depths limited to 15 by halving."""
    counts = np.concatenate([np.asarray(hist, dtype=np.int64), [1]])
    halvings = 0
    while True:
        lens = huffman_depths(counts)
        if lens.max() <= MAX_BITS:
            return lens, halvings
        counts = np.where(counts > 0, (counts + 1) >> 1, 0)
        halvings += 1


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> codes int [len(lens)], most significant bit first."""
    bl = np.bincount(lens, minlength=MAX_BITS + 2)
    bl[0] = 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for b in range(1, MAX_BITS + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = np.zeros(len(lens), dtype=np.int64)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _reverse(codes, lens):
    out = np.zeros_like(codes)
    for k in range(MAX_BITS):
        out |= ((codes >> k) & 1) << np.maximum(lens - 1 - k, 0)
    return np.where(lens > 0, out, 0)


def kraft(lens):
    """Sum of 2^-len over the used symbols, as an exact fraction of 2^15."""
    return int(sum(1 << (MAX_BITS - int(l)) for l in lens if l)), 1 << MAX_BITS


def block_bits(hist, lens):
    """Bits of one deflate block up to and including its end-of-block code."""
    return HEADER_BITS + int((np.asarray(hist, dtype=np.int64) * lens[:256]).sum()) + int(lens[256])


def deflate_block(data, final):
    """One block of the filtered stream -> the bytes of its dynamic block + the empty stored block."""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    hist = np.bincount(data, minlength=256)
    lens, _ = code_lengths(hist)
    rev = _reverse(canonical_codes(lens), lens)
    val, nb = [], []

    def put(v, n):
        val.append(v)
        nb.append(n)
    put(0, 1)                                             # BFINAL
    put(2, 2)                                             # BTYPE: dynamic
    put(0, 5)                                             # HLIT 257
    put(0, 5)                                             # HDIST 1
    put(15, 4)                                            # HCLEN 19
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        put(0 if sym >= 16 else 4, 3)
    rev4 = [int(f"{v:04b}"[::-1], 2) for v in range(16)]  # the code of length value v is v itself, sent high bit first
    for l in list(lens) + [0]:                            # 257 literal / length code lengths, one distance length 0
        put(rev4[int(l)], 4)
    assert sum(nb) == HEADER_BITS
    val = np.concatenate([np.asarray(val, dtype=np.int64), rev[data], [rev[256]], [1 if final else 0]])
    nb = np.concatenate([np.asarray(nb, dtype=np.int64), lens[data], [lens[256]], [3]])   # ..., end of block, stored header
    pos = np.concatenate([[0], np.cumsum(nb)])
    bits = np.zeros(-(-int(pos[-1]) // 8) * 8, dtype=np.uint8)
    for k in range(MAX_BITS):
        m = nb > k
        bits[pos[:-1][m] + k] = (val[m] >> k) & 1
    return np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(img, filt=ADAPTIVE):
    """uint8 (h, w, 3) -> the PNG file as bytes."""
    img = np.asarray(img)
    h, w, _ = img.shape
    stream, _ = filter_stream(img, filt)
    raw = stream.tobytes()
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    nblk = -(-len(raw) // BLOCK)
    for k in range(nblk):
        body = deflate_block(raw[k * BLOCK:(k + 1) * BLOCK], k == nblk - 1)
        if k == 0:
            body = b"\x78\x01" + body
        if k == nblk - 1:
            body += struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)
        out.append(chunk(b"IDAT", body))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def png_size(img, filt=ADAPTIVE):
    """len(encode(img, filt)) from the histograms and the code lengths of the blocks, without packing a bit."""
    stream, _ = filter_stream(img, filt)
    nblk = -(-len(stream) // BLOCK)
    total = 8 + 25 + 12 + 2 + 4                           # signature, IHDR, IEND, zlib header, Adler-32
    for k in range(nblk):
        hist = np.bincount(stream[k * BLOCK:(k + 1) * BLOCK], minlength=256)
        lens, _ = code_lengths(hist)
        total += 12 + (block_bits(hist, lens) + 3 + 7) // 8 + 4
    return total


def block_cap(nbytes):
    """Worst-case payload bytes of the IDAT of a block of `nbytes` filtered bytes (RCDM_PNG_SLOT for a full block's formula):
    an optimal code costs <= 9 bits a symbol (the flat 9-bit code is a prefix code); the limiter halves at most 4 times (a
    Huffman tree deeper than 15 needs a total count >= F(18) = 2584, and k halvings leave <= 32769 / 2^k + 257), which
    inflates the cost to <= 9 (n + 1 + 257 * 16) bits."""
    return 10 + (HEADER_BITS + 3 + 9 * (nbytes + 4113) + 7) // 8


def bound(h, w):
    """rcdm_png_bound of an h x w image."""
    total = h * (1 + 3 * w)
    nblk = -(-total // BLOCK)
    return 8 + 25 + 12 + sum(12 + block_cap(min(BLOCK, total - k * BLOCK)) for k in range(nblk))


def parse_chunks(data):
    """-> [(kind, payload, stored crc, zlib.crc32 of kind + payload)] of a PNG file; asserts the signature and the length."""
    assert data[:8] == SIGNATURE
    out, off = [], 8
    while off < len(data):
        n, = struct.unpack(">I", data[off:off + 4])
        kind, body = data[off + 4:off + 8], data[off + 8:off + 8 + n]
        crc, = struct.unpack(">I", data[off + 8 + n:off + 12 + n])
        out.append((kind, body, crc, zlib.crc32(kind + body) & 0xFFFFFFFF))
        off += 12 + n
    assert off == len(data) and out[-1][0] == b"IEND"
    return out


def cartoon(h, w, sigma, seed):
    """A procedural cartoon-like frame: flat discs over a gradient, Gaussian noise of `sigma` grey levels on top."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([80 + 100 * xx / w, 120 + 60 * yy / h, 200 - 80 * (xx + yy) / (h + w)], axis=2)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.25) * min(h, w)
        img[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rng.uniform(20, 235, size=3)
    if sigma > 0:
        img = img + rng.normal(0.0, sigma, size=img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
