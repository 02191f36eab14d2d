"""Plain Python / numpy restatement of the PNG reader (include/rcdm.h, "PNG, reading"; csrc/png_inflate.h):

  walk       the container: signature, chunk headers, IHDR / PLTE / IDAT positions (what rcdms_amd/image.py does on the host)
  inflate    zlib header, stored / fixed / dynamic blocks, Adler-32 — with the status codes of the header and the core's
             order of checks: bits past the stream's end read as zeros and are refused once consumed, every write is checked
             against `expect` first
  unfilter   the five filters at bpp 1 / 2 / 3 / 4, then RGB: grey replicated, alpha dropped, palette looked up (black beyond
             its end)
  Deflate    a small deflate WRITER: stored, fixed and dynamic blocks from a token list (literal ints, (length, distance)
             pairs, raw symbols for the corrupt files), code lengths by the two-queue Huffman of tests/png_oracle.py or given
  make_png, rechunk, set_height   files around a zlib stream, IDATs re-cut (zero-length ones included), CRCs always right

Nothing here is fast; the fixtures are small."""
import json
import os
import struct
import zlib

import numpy as np

from tests import png_oracle as P

OK, EZLIB, ETRUNC, EBLOCK, ESTORED, ECODES, ESYMBOL, EDISTANCE, EOVERRUN, EUNDERRUN, EADLER, EFILTER = range(12)
STATUS_NAMES = ["OK", "RCDM_PNG_EZLIB", "RCDM_PNG_ETRUNC", "RCDM_PNG_EBLOCK", "RCDM_PNG_ESTORED", "RCDM_PNG_ECODES",
                "RCDM_PNG_ESYMBOL", "RCDM_PNG_EDISTANCE", "RCDM_PNG_EOVERRUN", "RCDM_PNG_EUNDERRUN", "RCDM_PNG_EADLER",
                "RCDM_PNG_EFILTER"]
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in range(2)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ["small", "types", "cartoon0", "cartoon2", "far", "flat", "crafted", "corrupt"]


def golden(name):
    """tests/golden/pngd_<name>.npz -> [(fixture name, file bytes, status, uint8 (h, w, 3) pixels or None)], meta"""
    g = np.load(os.path.join(GOLD, f"pngd_{name}.npz"))
    out, f_at, p_at = [], 0, 0
    for nm, size, st, (h, w) in zip(g["names"], g["sizes"], g["status"], g["shapes"]):
        data = g["files"][f_at:f_at + size].tobytes()
        f_at += int(size)
        px = None
        if st == 0:
            px = g["pixels"][p_at:p_at + h * w * 3].reshape(h, w, 3)
            p_at += int(h * w * 3)
        out.append((str(nm), data, int(st), px))
    return out, json.loads(str(g["meta"]))


def written_goldens():
    """The files of every tests/golden/png_*.npz and pngm_*.npz (what rcdm_png_encode and its match mode write) with the
    pixels they were written from -> [(name, file bytes, uint8 (h, w, 3))]"""
    out = []
    for fn in sorted(os.listdir(GOLD)):
        if fn.startswith(("png_", "pngm_")) and fn.endswith(".npz"):
            g = np.load(os.path.join(GOLD, fn))
            ends = np.cumsum(g["sizes"])
            for i, (s, e) in enumerate(zip(g["sizes"], ends)):
                out.append((f"{fn[:-4]}[{i}]", g["files"][e - s:e].tobytes(), g["input"][i]))
    return out


# ------------------------------------------------------------------------------------------------ container
def walk(data):
    """-> dict(w, h, depth, color_type, interlace, idats [(offset, bytes)], plte (offset, bytes) or None); offsets of payloads."""
    assert data[:8] == P.SIGNATURE
    out = dict(w=None, idats=[], plte=None)
    off = 8
    while off + 12 <= len(data):
        n, = struct.unpack(">I", data[off:off + 4])
        kind = data[off + 4:off + 8]
        if kind == b"IHDR":
            w, h, depth, ct, _, _, il = struct.unpack(">IIBBBBB", data[off + 8:off + 21])
            out.update(w=w, h=h, depth=depth, color_type=ct, interlace=il)
        elif kind == b"PLTE":
            out["plte"] = (off + 8, n)
        elif kind == b"IDAT":
            out["idats"].append((off + 8, n))
        elif kind == b"IEND":
            break
        off += 12 + n
    return out


def zlib_stream(data):
    return b"".join(data[o:o + n] for o, n in walk(data)["idats"])


def make_png(w, h, color_type, z, plte=None, idat_sizes=None, extra=()):
    """A file around the zlib stream z; idat_sizes: the IDAT payload sizes in order, the rest of z goes into a last one."""
    out = [P.SIGNATURE, P.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color_type, 0, 0, 0))]
    out += [P.chunk(k, b) for k, b in extra]
    if plte is not None:
        out.append(P.chunk(b"PLTE", bytes(plte)))
    at = 0
    for n in list(idat_sizes or []):
        out.append(P.chunk(b"IDAT", z[at:at + n]))
        at += n
    out.append(P.chunk(b"IDAT", z[at:]))
    out.append(P.chunk(b"IEND", b""))
    return b"".join(out)


def _rebuild(data, z=None, h=None, idat_sizes=None):
    m = walk(data)
    plte = data[m["plte"][0]:m["plte"][0] + m["plte"][1]] if m["plte"] else None
    return make_png(m["w"], m["h"] if h is None else h, m["color_type"], zlib_stream(data) if z is None else z, plte, idat_sizes)


def rechunk(data, sizes):
    """The same file with its IDAT payload re-cut into chunks of `sizes` and one more for the rest."""
    return _rebuild(data, idat_sizes=sizes)


def set_height(data, h):
    return _rebuild(data, h=h)


def set_stream(data, z):
    return _rebuild(data, z=z)


# ------------------------------------------------------------------------------------------------ inflate
def _canon(lens, one_code_ok=True):
    """-> (status, table, maxlen): table[peeked maxlen bits] = symbol << 4 | length, 0 where no code owns the bits."""
    lens = np.asarray(lens, dtype=np.int64)
    count = np.bincount(lens, minlength=16)
    left, maxl = 1, 0
    for l in range(1, 16):
        left = (left << 1) - int(count[l])
        if left < 0:
            return ECODES, None, 0
        if count[l]:
            maxl = l
    if maxl and left > 0 and not (one_code_ok and maxl == 1):
        return ECODES, None, 0
    if maxl == 0:
        return OK, np.zeros(2, dtype=np.int64), 1
    codes = P.canonical_codes(lens)
    table = np.zeros(1 << maxl, dtype=np.int64)
    for s in np.flatnonzero(lens):
        l = int(lens[s])
        rev = int(f"{int(codes[s]):0{l}b}"[::-1], 2)
        table[rev::1 << l] = (int(s) << 4) | l
    return OK, table, maxl


def inflate(z, expect, blocks=None):
    """-> (status, bytes written so far); blocks: a list that receives [kind, matches, longest, farthest, overlapping] per block"""
    z = bytes(z)
    zbits = 8 * len(z)
    data = z + b"\0" * 8
    out = bytearray()
    p = 0                                                 # bits consumed

    def peek():
        return int.from_bytes(data[p >> 3:(p >> 3) + 4], "little") >> (p & 7)

    def bits(n):
        nonlocal p
        v = peek() & ((1 << n) - 1)
        p += n
        return v

    cmf, flg = bits(8), bits(8)
    if p > zbits:
        return ETRUNC, out
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or (flg & 0x20) or ((cmf << 8) | flg) % 31:
        return EZLIB, out
    while True:
        final, kind = bits(1), bits(2)
        if p > zbits:
            return ETRUNC, out
        if kind == 3:
            return EBLOCK, out
        blk = [kind, 0, 0, 0, 0]
        if blocks is not None:
            blocks.append(blk)
        if kind == 0:
            p += -p & 7
            n, nn = bits(16), bits(16)
            if p > zbits:
                return ETRUNC, out
            if n ^ 0xFFFF != nn:
                return ESTORED, out
            at = p >> 3
            if at + n > len(z):
                return ETRUNC, out
            if n > expect - len(out):
                return EOVERRUN, out
            out += z[at:at + n]
            p += 8 * n
        else:
            if kind == 1:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                nlit, ndist, ncl = bits(5) + 257, bits(5) + 1, bits(4) + 4
                if nlit > 286 or ndist > 30:
                    return ECODES, out
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = bits(3)
                if p > zbits:
                    return ETRUNC, out
                st, tab, ml = _canon(cl, one_code_ok=False)
                if st:
                    return ECODES, out
                lens = []
                while len(lens) < nlit + ndist:
                    e = int(tab[peek() & ((1 << ml) - 1)])
                    if not e:
                        return ECODES, out
                    p += e & 15
                    s, rep, v = e >> 4, 1, e >> 4
                    if s == 16:
                        if not lens:
                            return ECODES, out
                        v, rep = lens[-1], 3 + bits(2)
                    elif s == 17:
                        v, rep = 0, 3 + bits(3)
                    elif s == 18:
                        v, rep = 0, 11 + bits(7)
                    if p > zbits:
                        return ETRUNC, out
                    if len(lens) + rep > nlit + ndist:
                        return ECODES, out
                    lens += [v] * rep
                if lens[256] == 0:
                    return ECODES, out
                lit_lens, dist_lens = lens[:nlit], lens[nlit:]
            st1, lt, lm = _canon(lit_lens)
            st2, dt, dm = _canon(dist_lens)
            if st1 or st2:
                return ECODES, out
            lmask, dmask = (1 << lm) - 1, (1 << dm) - 1
            while True:
                e = int(lt[peek() & lmask])
                if not e:
                    return ESYMBOL, out
                p += e & 15
                sym = e >> 4
                if sym < 256:
                    if p > zbits:
                        return ETRUNC, out
                    if len(out) >= expect:
                        return EOVERRUN, out
                    out.append(sym)
                    continue
                if sym == 256:
                    if p > zbits:
                        return ETRUNC, out
                    break
                if sym >= 286:
                    return ESYMBOL, out
                L = LBASE[sym - 257] + bits(LEXT[sym - 257])
                e = int(dt[peek() & dmask])
                if not e:
                    return ESYMBOL, out
                p += e & 15
                ds = e >> 4
                if ds >= 30:
                    return ESYMBOL, out
                D = DBASE[ds] + bits(DEXT[ds])
                if p > zbits:
                    return ETRUNC, out
                if D > len(out):
                    return EDISTANCE, out
                if L > expect - len(out):
                    return EOVERRUN, out
                blk[1:] = [blk[1] + 1, max(blk[2], L), max(blk[3], D), blk[4] + (D < L)]
                if D >= L:
                    out += out[len(out) - D:len(out) - D + L]
                else:
                    seg = bytes(out[len(out) - D:])
                    out += (seg * (L // D + 1))[:L]
        if final:
            break
    if len(out) != expect:
        return EUNDERRUN, out
    p += -p & 7
    want = 0
    for _ in range(4):
        want = (want << 8) | bits(8)
    if p > zbits:
        return ETRUNC, out
    return (OK if want == (zlib.adler32(bytes(out)) & 0xFFFFFFFF) else EADLER), out


# ------------------------------------------------------------------------------------------------ filters, colour
def unfilter(raw, h, w, bpp):
    """raw: h * (1 + bpp w) inflated bytes -> (status, uint8 (h, w * bpp))"""
    S = 1 + bpp * w
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(h, S)
    if (rows[:, 0] > 4).any():
        return EFILTER, None
    out = np.zeros((h, bpp * w), dtype=np.uint8)
    prev = np.zeros(bpp * w, dtype=np.int64)
    for r in range(h):
        ft, x = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        else:
            cur = np.zeros(bpp * w, dtype=np.int64)
            xs, pv = x.tolist(), prev.tolist()
            cl = [0] * (bpp * w)
            for i in range(bpp * w):
                a = cl[i - bpp] if i >= bpp else 0
                b = pv[i]
                c = pv[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    q = a + b - c
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cl[i] = (xs[i] + pred) & 255
            cur = np.asarray(cl, dtype=np.int64)
        out[r] = cur
        prev = cur
    return OK, out


def to_rgb(px, w, color_type, plte=None):
    """(h, w * bpp) reconstructed bytes -> (h, w, 3)"""
    h = px.shape[0]
    v = px.reshape(h, w, BPP[color_type])
    if color_type in (2, 6):
        return np.ascontiguousarray(v[:, :, :3])
    if color_type in (0, 4):
        return np.repeat(v[:, :, :1], 3, axis=2)
    table = np.zeros((256, 3), dtype=np.uint8)
    pal = np.frombuffer(bytes(plte), dtype=np.uint8)
    n = min(len(pal) // 3, 256)
    table[:n] = pal[:3 * n].reshape(n, 3)
    return table[v[:, :, 0]]


def decode(data, order="rgb"):
    """A PNG file -> (status, uint8 (h, w, 3) or None)"""
    m = walk(data)
    bpp = BPP[m["color_type"]]
    assert m["depth"] == 8 and m["interlace"] == 0 and m["idats"]
    st, raw = inflate(zlib_stream(data), m["h"] * (1 + bpp * m["w"]))
    if st:
        return st, None
    st, px = unfilter(raw, m["h"], m["w"], bpp)
    if st:
        return st, None
    plte = data[m["plte"][0]:m["plte"][0] + m["plte"][1]] if m["plte"] else None
    rgb = to_rgb(px, m["w"], m["color_type"], plte)
    return OK, (rgb if order == "rgb" else np.ascontiguousarray(rgb[:, :, ::-1]))


# ------------------------------------------------------------------------------------------------ a deflate writer
def _length_symbol(L):
    s = max(k for k in range(29) if LBASE[k] <= L) if L < 258 else 28
    return 257 + s, L - LBASE[s], LEXT[s]


def _dist_symbol(D):
    s = max(k for k in range(30) if DBASE[k] <= D)
    return s, D - DBASE[s], DEXT[s]


class Deflate:
    """Blocks from tokens: an int is a literal, (L, D) a match, ("lit", s) / ("dist", s) a raw symbol of that code with no
    extra bits, ("bits", v, n) raw bits."""

    def __init__(self):
        self.val, self.nb = [], []

    def put(self, v, n):
        self.val.append(int(v))
        self.nb.append(int(n))

    def _align(self):
        self.put(0, -sum(self.nb) & 7)

    def stored(self, data, final=False, nlen=None):
        self.put(1 if final else 0, 1)
        self.put(0, 2)
        self._align()
        n = len(data)
        self.put(n, 16)
        self.put((n ^ 0xFFFF) if nlen is None else nlen, 16)
        for b in bytes(data):
            self.put(b, 8)
        return self

    def reserved(self, final=True):
        self.put(1 if final else 0, 1)
        self.put(3, 2)
        return self

    def _symbols(self, tokens):
        """-> [(code, symbol, extra value, extra bits)] with code 0 = literal / length, 1 = distance; ends with end-of-block"""
        out = []
        for t in tokens:
            if isinstance(t, (int, np.integer)):
                out.append((0, int(t), 0, 0))
            elif t[0] == "lit":
                out.append((0, t[1], 0, 0))
            elif t[0] == "dist":
                out.append((1, t[1], 0, 0))
            elif t[0] == "bits":
                out.append((2, 0, t[1], t[2]))
            else:
                s, ev, eb = _length_symbol(t[0])
                out.append((0, s, ev, eb))
                s, ev, eb = _dist_symbol(t[1])
                out.append((1, s, ev, eb))
        out.append((0, 256, 0, 0))
        return out

    def _emit(self, syms, lit_lens, dist_lens):
        lens = (np.asarray(lit_lens, dtype=np.int64), np.asarray(dist_lens, dtype=np.int64))
        codes = tuple(P.canonical_codes(l) if l.max() > 0 else l for l in lens)
        for which, s, ev, eb in syms:
            if which < 2:
                l = int(lens[which][s])
                assert l > 0, f"symbol {s} of code {which} has no code"
                self.put(int(f"{int(codes[which][s]):0{l}b}"[::-1], 2), l)
            self.put(ev, eb)

    def fixed(self, tokens, final=False):
        self.put(1 if final else 0, 1)
        self.put(1, 2)
        self._emit(self._symbols(tokens), FIXED_LIT, FIXED_DIST)
        return self

    def dynamic(self, tokens, final=False, lit_lens=None, dist_lens=None):
        """Code lengths from the tokens' histogram (two-queue Huffman, no limiter: small blocks) unless given.  The header
        sends every length with the flat 4-bit code-length code (no repeat codes), as rcdm_png_encode does."""
        syms = self._symbols(tokens)
        if lit_lens is None:
            hist = np.bincount([s for w, s, _, _ in syms if w == 0], minlength=286)
            lit_lens = P.huffman_depths(hist) if (hist > 0).sum() > 1 else (hist > 0).astype(np.int64)
            assert lit_lens.max() <= 15
        if dist_lens is None:
            hist = np.bincount([s for w, s, _, _ in syms if w == 1], minlength=1)
            dist_lens = P.huffman_depths(hist) if (hist > 0).sum() > 1 else (hist > 0).astype(np.int64)
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        while len(lit_lens) > 257 and lit_lens[-1] == 0:
            lit_lens.pop()
        while len(dist_lens) > 1 and dist_lens[-1] == 0:
            dist_lens.pop()
        self.put(1 if final else 0, 1)
        self.put(2, 2)
        self.put(len(lit_lens) - 257, 5)
        self.put(len(dist_lens) - 1, 5)
        self.put(15, 4)
        for s in CL_ORDER:
            self.put(0 if s >= 16 else 4, 3)
        for l in lit_lens + dist_lens:
            self.put(int(f"{int(l):04b}"[::-1], 2), 4)
        self._emit(syms, lit_lens + [0] * (286 - len(lit_lens)), dist_lens + [0] * (30 - len(dist_lens)))
        return self

    def tobytes(self):
        bits = np.zeros(-(-sum(self.nb) // 8) * 8, dtype=np.uint8)
        at = 0
        for v, n in zip(self.val, self.nb):
            for k in range(n):
                bits[at + k] = (v >> k) & 1
            at += n
        return np.packbits(bits, bitorder="little").tobytes()


def zlib_wrap(deflate_bytes, raw):
    return b"\x78\x01" + deflate_bytes + struct.pack(">I", zlib.adler32(bytes(raw)) & 0xFFFFFFFF)
