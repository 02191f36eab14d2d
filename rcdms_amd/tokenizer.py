"""CLIP tokenizer on the HIP path: captions go up as bytes, token ids are born on the device (rcdm_clip_tokenize).

`ClipTokenizer` stands where the two pipelines hold the caller's `transformers.CLIPTokenizer`: it answers the call they make —
`tok(texts, padding="max_length", max_length=L, truncation=..., return_tensors="pt")` — and the driver's `add_tokens([...])` /
`len(tok)` (stage2_batchtest_rcdms_model.py:203-205), and needs nothing from `transformers`.  What it computes is the `tokenizers`
backend of transformers 5.x, step by step in include/rcdm.h ("CLIP tokenizer") and restated in tests/tokenizer_oracle.py.
PARITY: pinned to that backend on synthetic vocabularies (tests/golden/tok_*.npz, minted by tools/mint_tokenizer_golden.py);
never run on the real CLIP vocab.json / merges.txt, which the repository does not hold.

Limits, all raised as ValueError before anything is launched: ASCII captions of at most 1024 bytes (the data sets' captions are
ASCII; NFC and the \\p{L} / \\p{N} tables are out of scope), padding="max_length" and return_tensors="pt" only, at most 64 added
tokens of at most 32 bytes each, without whitespace.

One call is one upload (offsets and bytes in one pinned buffer) and one launch.  The result's four fields are device tensors:
input_ids and attention_mask (int64, what transformers returns), lengths (int32 (n): tokens + 2, untruncated) and pool_index
(int32 (n, 2): position of the row's largest id, position of its first eos) — what CLIPTextEncoder.forward(pool_index=...,
ids_checked=True) takes in place of its own device -> host copy.  With truncation=False the lengths are read back once and a
caption that does not fit raises ValueError (transformers would return a longer row, which the text encoder's position table
refuses anyway).  The tables (pair hash, byte tables, added tokens) are built once on the host, cached per device and rebuilt
only by add_tokens.  No CPU path: hip.RcdmError without a GPU."""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import hip

BOS, EOS = "<|startoftext|>", "<|endoftext|>"
_NONE = 0xFFFFFFFF


def bytes_to_unicode():
    """GPT-2's byte -> printable symbol map, the alphabet of vocab.json."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    out, n = {}, 0
    for b in range(256):
        if b in keep:
            out[b] = chr(b)
        else:
            out[b] = chr(256 + n)
            n += 1
    return out


def pair_hash(a, b):
    """rcdm_tok_pair_hash on uint32 arrays."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = ((a * np.uint64(0x9E3779B1)) & m) ^ ((b * np.uint64(0x85EBCA6B)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    return h.astype(np.uint32)


def build_pair_table(a, b, merged):
    """(a[i], b[i]) -> (rank i, merged[i]) as the open-addressing table of rcdm_tok_pair: (slots, 4) uint32, slots a power of two
    >= 2 n (at most half full), linear probing, empty slots a == 0xFFFFFFFF.  Of equal pairs the first (lowest rank) stays."""
    n = len(a)
    slots = 2
    while slots < 2 * n:
        slots *= 2
    table = np.zeros((slots, 4), dtype=np.uint32)
    table[:, 0] = _NONE
    home = (pair_hash(a, b) & np.uint32(slots - 1)).tolist()
    key = table[:, 0].tolist()
    other = [0] * slots
    a, b, merged = (np.asarray(x).tolist() for x in (a, b, merged))
    for r in range(n):
        at = home[r]
        while key[at] != _NONE and not (key[at] == a[r] and other[at] == b[r]):
            at = (at + 1) & (slots - 1)
        if key[at] == _NONE:
            key[at], other[at] = a[r], b[r]
            table[at] = (a[r], b[r], r, merged[r])
    return table


class TokenizerOutput(dict):
    """input_ids, attention_mask, lengths, pool_index: answers both `.name` and `["name"]`."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def _token_text(t):
    return t["content"] if isinstance(t, dict) else t


class ClipTokenizer:
    def __init__(self, vocab, merges, model_max_length=77, pad_token=None, bos_token=BOS, eos_token=EOS):
        """vocab: token -> id (vocab.json); merges: "a b" strings or (a, b) pairs in rank order (merges.txt without its header);
        pad_token: a vocabulary entry, default eos_token (CLIP's own configuration)."""
        self.vocab = dict(vocab)
        self.model_max_length = int(model_max_length)
        self.bos_token, self.eos_token = bos_token, eos_token
        self.pad_token = eos_token if pad_token is None else pad_token
        for t in (self.bos_token, self.eos_token, self.pad_token):
            if t not in self.vocab:
                raise ValueError(f"special token {t!r} is not in the vocabulary")
        self.bos_token_id, self.eos_token_id, self.pad_token_id = (self.vocab[t] for t in (bos_token, eos_token, self.pad_token))
        sym = bytes_to_unicode()
        try:
            self._byte_ids = np.array([self.vocab[sym[b]] for b in range(256)] + [self.vocab[sym[b] + "</w>"] for b in range(256)],
                                      dtype=np.int32)
        except KeyError as e:
            raise ValueError(f"the vocabulary lacks the byte symbol {e.args[0]!r}: not a byte-level CLIP vocabulary") from None
        pairs = [tuple(m.split(" ")) if isinstance(m, str) else tuple(m) for m in merges]
        if len(pairs) >= hip.TOK_MAX_RANK:
            raise ValueError(f"{len(pairs)} merges: the kernel's keys hold ranks below {hip.TOK_MAX_RANK}")
        try:
            cols = [[self.vocab[a] for a, _ in pairs], [self.vocab[b] for _, b in pairs], [self.vocab[a + b] for a, b in pairs]]
        except (KeyError, ValueError) as e:
            raise ValueError(f"merges name a token the vocabulary lacks, or a line is not 'a b': {e}") from None
        self._pairs = build_pair_table(*(np.array(c, dtype=np.uint32) for c in cols))
        self._specials = [(bos_token, self.bos_token_id)] + ([(eos_token, self.eos_token_id)] if eos_token != bos_token else [])
        for t, _ in self._specials:
            self._check_added_text(t)
        self._added = []                    # (lower-cased text, id) in the order of add_tokens
        self._size = max(self.vocab.values()) + 1
        self._version = 0                   # bumped by add_tokens: the device copies are rebuilt
        self._dev = {}                      # device -> (version, buffer, (pairs, byte_ids, added) byte offsets)
        self.device = torch.device("cuda")

    # ---- construction -------------------------------------------------------------------------------------------------
    @classmethod
    def from_files(cls, vocab_json, merges_txt, **kw):
        with open(vocab_json, encoding="utf-8") as f:
            vocab = json.load(f)
        with open(merges_txt, encoding="utf-8") as f:
            lines = f.read().split("\n")
        if lines and lines[0].startswith("#version"):
            lines = lines[1:]
        return cls(vocab, [ln for ln in lines if ln.strip()], **kw)

    @classmethod
    def from_pretrained(cls, path, subfolder=None):
        """A local directory holding vocab.json and merges.txt, and tokenizer_config.json / added_tokens.json where present.
        Nothing is fetched."""
        d = os.path.join(path, subfolder) if subfolder else path
        if not os.path.isdir(d):
            raise FileNotFoundError(f"{d}: from_pretrained reads a local directory only")
        kw, cfg_path, added_path = {}, os.path.join(d, "tokenizer_config.json"), os.path.join(d, "added_tokens.json")
        if os.path.exists(cfg_path):
            with open(cfg_path, encoding="utf-8") as f:
                cfg = json.load(f)
            for k in ("bos_token", "eos_token", "pad_token"):
                if cfg.get(k) is not None:
                    kw[k] = _token_text(cfg[k])
            if isinstance(cfg.get("model_max_length"), int) and cfg["model_max_length"] < 1 << 20:
                kw["model_max_length"] = cfg["model_max_length"]
        tok = cls.from_files(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"), **kw)
        if os.path.exists(added_path):
            with open(added_path, encoding="utf-8") as f:
                added = json.load(f)
            for t, i in sorted(added.items(), key=lambda kv: kv[1]):
                if t in (tok.bos_token, tok.eos_token):
                    continue
                tok.add_tokens([t])
                if tok._added[-1][1] != i:
                    raise ValueError(f"added_tokens.json gives {t!r} id {i}, add_tokens assigns {tok._added[-1][1]}")
        return tok

    @staticmethod
    def _check_added_text(t):
        if not isinstance(t, str):
            raise TypeError(f"added tokens are strings, got {type(t).__name__}")
        b = t.encode("utf-8")
        if not b or len(b) > hip.TOK_MAX_ADDED_LEN or any(c >= 128 or c in (9, 10, 11, 12, 13, 32) for c in b):
            raise ValueError(f"added token {t!r}: 1 to {hip.TOK_MAX_ADDED_LEN} ASCII bytes without whitespace")

    def add_tokens(self, tokens):
        """The driver's add_tokens(["fred", ...]): each token is from now on matched before anything else, on the lower-cased
        text and also inside words, and is one id.  -> the count the backend returns: every token but a repeat of an earlier
        one or of a special string.  A token whose exact text is a vocabulary entry keeps that id; the others get len(self),
        len(self) + 1, ..."""
        tokens = [tokens] if isinstance(tokens, str) else list(tokens)
        for t in tokens:
            self._check_added_text(t)
        fresh = []
        for t in tokens:
            key = t.lower()
            if key in (k for k, _ in self._added + fresh) or t in (s for s, _ in self._specials):
                continue
            fresh.append((key, self.vocab[t] if t in self.vocab else self._size + sum(1 for _, i in fresh if i >= self._size)))
        if len(self._added) + len(fresh) > hip.TOK_MAX_ADDED:
            raise ValueError(f"{len(self._added) + len(fresh)} added tokens: at most {hip.TOK_MAX_ADDED}")
        self._added += fresh
        self._size += sum(1 for _, i in fresh if i >= self._size)
        if fresh:
            self._version += 1
        return len(fresh)

    def __len__(self):
        return self._size

    def to(self, device):
        self.device = torch.device(device)
        return self

    # ---- tables -------------------------------------------------------------------------------------------------------
    def host_tables(self):
        """-> (pairs (slots, 4) uint32, byte_ids (512) int32, added (rows, 48) uint8: rcdm_tok_added records, specials first)."""
        rows = np.zeros((len(self._specials) + len(self._added), C.sizeof(hip.TokAdded)), dtype=np.uint8)
        for r, ((t, i), special) in enumerate([(s, 1) for s in self._specials] + [(a, 0) for a in self._added]):
            b = t.encode("ascii")
            rows[r, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            rows[r, 32:48] = np.array([len(b), i, special, 0], dtype=np.int32).view(np.uint8)
        return self._pairs, self._byte_ids, rows

    def _tables(self, device):
        """The three tables in one device buffer (one upload), cached until add_tokens."""
        have = self._dev.get(device)
        if have is None or have[0] != self._version:
            pairs, byte_ids, rows = self.host_tables()
            parts = [pairs.view(np.uint8).reshape(-1), byte_ids.view(np.uint8), rows.reshape(-1)]     # sizes: multiples of 16
            offs = np.cumsum([0] + [p.size for p in parts])
            buf = torch.from_numpy(np.concatenate(parts)).to(device)
            assert buf.data_ptr() % 16 == 0
            have = self._dev[device] = (self._version, buf, tuple(int(o) for o in offs[:3]))
        return have[1], have[2]

    # ---- the call -----------------------------------------------------------------------------------------------------
    @staticmethod
    def pack_texts(texts):
        """-> (offsets int32 (n + 1), bytes uint8): ValueError for a caption that is not ASCII or longer than the cap."""
        try:                                  # the common case in three passes over the whole batch, no Python loop per caption
            raw = "".join(texts).encode("ascii")
            lens = np.fromiter(map(len, texts), count=len(texts), dtype=np.int64)
        except (TypeError, UnicodeEncodeError):
            raw, lens = None, None
        if raw is None or lens.max(initial=0) > hip.TOK_MAX_CAPTION:
            for r, t in enumerate(texts):     # something is wrong: find it and name it
                if not isinstance(t, str):
                    raise TypeError(f"caption {r} is {type(t).__name__}, not str")
                if not t.isascii():
                    raise ValueError(f"caption {r} ({t!r}) is not ASCII: the HIP tokenizer covers ASCII captions only")
                if len(t) > hip.TOK_MAX_CAPTION:
                    raise ValueError(f"caption {r} is {len(t)} bytes, the cap is {hip.TOK_MAX_CAPTION}: {t[:60]!r}...")
        offsets = np.zeros(len(texts) + 1, dtype=np.int32)
        np.cumsum(lens, out=offsets[1:])
        return offsets, np.frombuffer(raw, dtype=np.uint8)

    @staticmethod
    def check_lengths(texts, lengths, max_length):
        """truncation=False: ValueError naming the first caption whose row (both specials counted) is longer than max_length."""
        for r, n in enumerate(lengths):
            if n < 0:
                raise RuntimeError(f"the kernel refused caption {r} ({texts[r]!r}) that the host checks passed")
            if n > max_length:
                raise ValueError(f"caption {r} ({texts[r]!r}) is {int(n)} tokens with both specials, max_length is {max_length} "
                                 f"and truncation is off")

    def desc(self, n, max_length, truncation, text_bytes, ld=None):
        return hip.TokenizeDesc(ld=max_length if ld is None else ld, text_bytes=text_bytes, n=n, max_length=max_length,
                                truncation=int(bool(truncation)), bos_id=self.bos_token_id, eos_id=self.eos_token_id,
                                pad_id=self.pad_token_id, n_added=len(self._specials) + len(self._added),
                                pair_slots=self._pairs.shape[0])

    def launch(self, offsets, text, max_length, truncation, out=None):
        """Upload (one pinned buffer: offsets, then bytes) and launch on the current stream.  out: optional preallocated
        (input_ids, attention_mask, lengths, pool_index) device tensors; the rows of the first two may be strided."""
        device = self.device if self.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        n = len(offsets) - 1
        head = 4 * (n + 1)
        staged = torch.empty(head + max(text.size, 1), dtype=torch.uint8, pin_memory=True)
        staged[:head] = torch.from_numpy(offsets.view(np.uint8))
        if text.size:
            staged[head:head + text.size] = torch.from_numpy(text.copy())
        with torch.cuda.device(device):               # the launch goes to this device's current stream
            return self._launch_on(device, staged, head, n, int(text.size), max_length, truncation, out)

    def _launch_on(self, device, staged, head, n, text_bytes, max_length, truncation, out):
        up = staged.to(device, non_blocking=True)
        tables, (o_pairs, o_bytes, o_rows) = self._tables(device)
        if out is None:
            out = (torch.empty(n, max_length, dtype=torch.int64, device=device), torch.empty(n, max_length, dtype=torch.int64, device=device),
                   torch.empty(n, dtype=torch.int32, device=device), torch.empty(n, 2, dtype=torch.int32, device=device))
        ids, mask, lengths, pool = out
        assert ids.stride(0) == mask.stride(0) and ids.stride(1) == mask.stride(1) == 1
        d = self.desc(n, max_length, truncation, text_bytes, ld=ids.stride(0))
        base = tables.data_ptr()
        hip.clip_tokenize(d, up.data_ptr() + head, up.data_ptr(), base + o_bytes, base + o_rows if d.n_added else 0, base + o_pairs,
                          ids.data_ptr(), mask.data_ptr(), lengths.data_ptr(), pool.data_ptr())
        return TokenizerOutput(input_ids=ids, attention_mask=mask, lengths=lengths, pool_index=pool)

    def __call__(self, text, padding=None, max_length=None, truncation=False, return_tensors=None):
        if padding != "max_length":
            raise ValueError(f"padding={padding!r}: the HIP tokenizer pads to max_length only")
        if return_tensors != "pt":
            raise ValueError(f"return_tensors={return_tensors!r}: the HIP tokenizer returns device torch tensors (\"pt\") only")
        texts = [text] if isinstance(text, str) else list(text)
        max_length = self.model_max_length if max_length is None else int(max_length)
        if not texts:
            raise ValueError("no captions")
        if not 2 <= max_length <= hip.TOK_MAX_CAPTION + 2 or len(texts) > hip.TOK_MAX_CAPTIONS:
            raise ValueError(f"max_length {max_length} outside 2 .. {hip.TOK_MAX_CAPTION + 2}, or more than {hip.TOK_MAX_CAPTIONS} captions")
        offsets, raw = self.pack_texts(texts)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise hip.RcdmError(f"ClipTokenizer runs on the HIP path only (device {self.device}, no CPU path)")
        out = self.launch(offsets, raw, max_length, truncation)
        if not truncation:
            self.check_lengths(texts, out.lengths.cpu().tolist(), max_length)
        return out

    # ---- for tools/tokenize_host.cpp ----------------------------------------------------------------------------------
    def dump(self, path, texts, max_length, truncation, expect=None):
        """One call's inputs as raw arrays, the file tools/tokenize_host.cpp reads: 10 int32 (magic, n, max_length, truncation,
        bos, eos, pad, rows, slots, text bytes), then offsets, byte_ids, the added rows, the pair slots, the text, and with
        `expect` (input_ids (n, max_length)) the expected ids as int64."""
        offsets, raw = self.pack_texts(texts)
        pairs, byte_ids, rows = self.host_tables()
        head = np.array([0x544F4B31, len(texts), max_length, int(bool(truncation)), self.bos_token_id, self.eos_token_id,
                         self.pad_token_id, rows.shape[0], pairs.shape[0], raw.size], dtype=np.int32)
        with open(path, "wb") as f:
            for part in (head, offsets, byte_ids, rows, pairs, raw):
                f.write(np.ascontiguousarray(part).tobytes())
            if expect is not None:
                f.write(np.ascontiguousarray(expect, dtype=np.int64).tobytes())
