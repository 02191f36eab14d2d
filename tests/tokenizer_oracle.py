"""Pure-Python restatement of what rcdms_amd/tokenizer.py computes: transformers.CLIPTokenizer (the `tokenizers` backend of
transformers 5.x) on ASCII captions, in the five steps of include/rcdm.h, "CLIP tokenizer".  Lists and dicts only, one
caption at a time: the yardstick of the goldens (tools/mint_tokenizer_golden.py refuses to write a file unless this module
reproduces every id transformers returned), of tools/tokenize_host.cpp and of the kernel.

  1. added tokens: the special strings on the raw text (case-sensitive), then the tokens of add_tokens on the lower-cased text of
     each stretch between them, also inside words; leftmost-longest, non-overlapping, one id per match
  2. normalise: lower-case (whitespace runs only separate words, so collapsing them changes nothing here)
  3. split: 's|'t|'re|'ve|'m|'ll|'d|[a-z]+|[0-9]|[^\\s a-z 0-9]+ in order, whitespace (9-13, 32) dropped
  4. byte-level BPE per word: the last symbol carries </w>; apply the ONE live pair of lowest rank, leftmost first, until no
     live pair has a merge
  5. frame: bos, tokens, eos, pad up to max_length; mask 1 through eos
"""
import functools
import os
import types

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ["english", "out_of_order", "repeated", "random0", "random1", "added", "shapes"]
BOS, EOS = "<|startoftext|>", "<|endoftext|>"
SPACE = frozenset((9, 10, 11, 12, 13, 32))
CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")        # the regex's order: the first that matches is taken


def bytes_to_unicode():
    """GPT-2's byte -> printable symbol map (public: openai/gpt-2 encoder.py)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    out, n = {}, 0
    for b in range(256):
        if b in keep:
            out[b] = chr(b)
        else:
            out[b] = chr(256 + n)
            n += 1
    return out


BYTE_SYMBOL = bytes_to_unicode()


def base_vocab():
    """The 512 entries every vocabulary here starts with, in CLIP's order: the byte symbols in the order of the real file
    (printable first), then the same with </w>."""
    syms = [chr(b) for b in list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))]
    syms += [BYTE_SYMBOL[b] for b in range(256) if BYTE_SYMBOL[b] not in syms]
    return syms + [s + "</w>" for s in syms]


def make_vocab(merges, specials=(BOS, EOS)):
    """token -> id: base_vocab(), one entry per merge (a + b) in merge order, then the special strings."""
    toks = base_vocab() + [a + b for a, b in merges] + list(specials)
    assert len(set(toks)) == len(toks), "two merges produce the same token"
    return {t: i for i, t in enumerate(toks)}


def _lower(c):
    return c + 32 if 65 <= c <= 90 else c


def _cls(c):
    """0 whitespace, 1 letter, 2 digit, 3 anything else (after lower-casing)."""
    return 0 if c in SPACE else 1 if 97 <= c <= 122 else 2 if 48 <= c <= 57 else 3


def split_words(b):
    """Step 3 on lower-cased bytes -> list of words (bytes)."""
    words, p, n = [], 0, len(b)
    while p < n:
        k = _cls(b[p])
        if k == 0:
            p += 1
            continue
        q = 0
        if b[p] == 39:
            for c in CONTRACTIONS:
                if b.startswith(c.encode(), p):
                    q = p + len(c)
                    break
        if not q:
            q = p + 1
            while k != 2 and q < n and _cls(b[q]) == k:        # a run of letters or of other bytes; a digit stands alone
                q += 1
        words.append(b[p:q])
        p = q
    return words


class Oracle:
    def __init__(self, vocab, merges, added=(), bos=BOS, eos=EOS, pad=None):
        self.vocab = dict(vocab)
        self.rank = {}
        for r, (a, b) in enumerate(merges):
            self.rank.setdefault((self.vocab[a], self.vocab[b]), (r, self.vocab[a + b]))
        self.bos_id, self.eos_id = self.vocab[bos], self.vocab[eos]
        self.pad_id = self.eos_id if pad is None else self.vocab[pad]
        self.special = [(bos.encode(), self.bos_id), (eos.encode(), self.eos_id)]
        self.added = []                       # (lower-cased bytes, id)
        self.size = max(self.vocab.values()) + 1
        self.add_tokens(added)

    def __len__(self):
        return self.size

    def add_tokens(self, tokens):
        """-> how many were taken (the backend's count): every token but a repeat of an earlier added one or of a special string.
        A token whose exact text is a vocabulary entry keeps that entry's id (and is still matched as an added token, inside
        words too); the others get the next free ids."""
        new = 0
        for t in tokens:
            key = t.lower().encode("ascii")
            if any(key == k for k, _ in self.added) or t in (s.decode() for s, _ in self.special):
                continue
            if t in self.vocab:
                self.added.append((key, self.vocab[t]))
            else:
                self.added.append((key, self.size))
                self.size += 1
            new += 1
        return new

    # ---- steps 1-4 ----
    @staticmethod
    def _matches(text, table, fold):
        """Leftmost-longest non-overlapping matches of the table's strings -> [(start, end, id)]."""
        out, p, n = [], 0, len(text)
        probe = bytes(_lower(c) for c in text) if fold else text
        while p < n:
            best = None
            for s, i in table:
                if probe.startswith(s, p) and (best is None or len(s) > len(best[0])):
                    best = (s, i)
            if best is None:
                p += 1
            else:
                out.append((p, p + len(best[0]), best[1]))
                p += len(best[0])
        return out

    def _bpe(self, word):
        syms = [self.vocab[BYTE_SYMBOL[c]] for c in word[:-1]] + [self.vocab[BYTE_SYMBOL[word[-1]] + "</w>"]]
        while True:
            best = None
            for i in range(len(syms) - 1):
                m = self.rank.get((syms[i], syms[i + 1]))
                if m is not None and (best is None or m[0] < best[0]):
                    best = (m[0], i, m[1])
            if best is None:
                return syms
            syms[best[1]:best[1] + 2] = [best[2]]

    def _plain(self, text):
        out = []
        for w in split_words(bytes(_lower(c) for c in text)):
            out += self._bpe(w)
        return out

    def _stretch(self, text):
        out, at = [], 0
        for s, e, i in self._matches(text, self.added, True):
            out += self._plain(text[at:s]) + [i]
            at = e
        return out + self._plain(text[at:])

    def tokens(self, text):
        """Caption -> ids without bos / eos."""
        b = text.encode("ascii") if isinstance(text, str) else bytes(text)
        if any(c >= 128 for c in b):
            raise ValueError(f"caption {text!r} is not ASCII")
        out, at = [], 0
        for s, e, i in self._matches(b, self.special, False):
            out += self._stretch(b[at:s]) + [i]
            at = e
        return out + self._stretch(b[at:])

    # ---- step 5 ----
    def __call__(self, texts, max_length=77, truncation=True):
        """-> dict of input_ids, attention_mask (int64 (n, max_length)), lengths (int32 (n)), pool_index (int32 (n, 2): argmax
        of the row, first eos)."""
        n = len(texts)
        ids = np.full((n, max_length), self.pad_id, dtype=np.int64)
        mask = np.zeros((n, max_length), dtype=np.int64)
        lengths = np.zeros(n, dtype=np.int32)
        for r, t in enumerate(texts):
            toks = self.tokens(t)
            lengths[r] = len(toks) + 2
            if len(toks) + 2 > max_length:
                if not truncation:
                    raise ValueError(f"caption {r} ({t!r}) is {len(toks) + 2} tokens with both specials, max_length is {max_length}")
                toks = toks[:max_length - 2]
            row = [self.bos_id] + toks + [self.eos_id]
            ids[r, :len(row)] = row
            mask[r, :len(row)] = 1
        pool = np.stack([ids.argmax(axis=1), (ids == self.eos_id).argmax(axis=1)], axis=1).astype(np.int32)
        return dict(input_ids=ids, attention_mask=mask, lengths=lengths, pool_index=pool)


# ---- the goldens ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden(name):
    """tests/golden/tok_<name>.npz -> vocab, merges [(a, b)], added [str], texts [str], max_lengths [int], lengths, and per
    max_length L: ids[L], mask[L] (transformers' rows, truncation on) and pool[L] (argmax of the row, first eos)."""
    g = np.load(os.path.join(GOLDEN_DIR, f"tok_{name}.npz"))
    raw, off = g["text"].tobytes(), g["offsets"]
    out = types.SimpleNamespace(name=name, vocab={str(t): i for i, t in enumerate(g["tokens"])},
                                merges=[tuple(str(m).split(" ")) for m in g["merges"]], added=[str(a) for a in g["added"]],
                                texts=[raw[off[i]:off[i + 1]].decode("ascii") for i in range(len(off) - 1)],
                                max_lengths=[int(L) for L in g["max_lengths"]], lengths=g["lengths"], ids={}, mask={}, pool={})
    eos = out.vocab[EOS]
    for L in out.max_lengths:
        ids = out.ids[L] = g[f"ids_{L}"]
        out.mask[L] = g[f"mask_{L}"]
        out.pool[L] = np.stack([ids.argmax(axis=1), (ids == eos).argmax(axis=1)], axis=1).astype(np.int32)
    return out


def fits(g, L):
    """Rows of golden g that fit max_length L untruncated: what truncation=False must reproduce."""
    return [r for r in range(len(g.texts)) if g.lengths[r] <= L]
