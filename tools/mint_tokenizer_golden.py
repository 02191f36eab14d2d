"""Mint tests/golden/tok_*.npz: synthetic vocabularies, captions, and the ids transformers.CLIPTokenizer (the `tokenizers`
backend) returns for them.  No real CLIP vocabulary is used: the tables are built here from a seed.  A file is written only if
tests/tokenizer_oracle.py reproduces every id, mask and length — the goldens pin the oracle to transformers, the oracle pins
the host core and the kernel.

  python tools/mint_tokenizer_golden.py [--out tests/golden]

Each file holds data only: `tokens` (the vocabulary in id order), `merges` ("a b" per line), `added` (strings handed to
add_tokens, in order), the captions as `text` (uint8) + `offsets` (int32, n + 1), `max_lengths`, and per max_length L the
arrays `ids_L`, `mask_L` (int64 (n, L), truncation on) plus `lengths` (int32, untruncated, both specials counted)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tokenizer_oracle as O  # noqa: E402

NAMES = ["pororo", "loopy", "eddy", "crong", "poby", "petty", "harry", "rody", "tongtong", "fred", "wilma", "barney", "betty",
         "pebbles", "dino", "slate", "bammbamm"]
WORDS = ("the a an and is are was were in on at to of with from into over under near behind holding looking standing sitting "
         "walking talking running jumping laughing smiling waving pointing cooking eating sleeping reading playing house room "
         "kitchen snow forest village table chair window door car rock stone dinosaur friend friends everyone someone they he "
         "she it his her their big small happy sad angry surprised red blue green white black wearing hat shirt dress outside "
         "inside then while when because very together again today tomorrow something nothing front back left right side "
         "says said tells asks thinks wants makes takes gives goes comes sees hears knows about after before there here").split()


def train_bpe(words, n_merges):
    """A plain BPE trainer over a word list (every word counted once): the most frequent adjacent pair, ties by the pair's
    text, merged everywhere.  -> [(a, b)] in training order, as many as the list gives up to n_merges."""
    seqs = [[O.BYTE_SYMBOL[c] for c in w.encode()[:-1]] + [O.BYTE_SYMBOL[w.encode()[-1]] + "</w>"] for w in sorted(set(words))]
    merges = []
    while len(merges) < n_merges:
        count = {}
        for s in seqs:
            for p in zip(s, s[1:]):
                count[p] = count.get(p, 0) + 1
        if not count:
            break
        a, b = min(count, key=lambda p: (-count[p], p))
        merges.append((a, b))
        for s in seqs:
            i = 0
            while i < len(s) - 1:
                if s[i] == a and s[i + 1] == b:
                    s[i:i + 2] = [a + b]
                else:
                    i += 1
    return merges


def random_merges(rng, symbols, n, merges=()):
    """n more merges in trained order over `symbols` (plain byte symbols): each joins two tokens that exist when it is made
    (a left part never carries </w>), and no two merges produce the same token."""
    merges = list(merges)
    left = [s for s in symbols] + [a + b for a, b in merges if not (a + b).endswith("</w>")]
    right = left + [s + "</w>" for s in symbols] + [a + b for a, b in merges if (a + b).endswith("</w>")]
    made = set(left) | set(right)
    want = len(merges) + n
    while len(merges) < want:
        a, b = left[rng.randint(len(left))], right[rng.randint(len(right))]
        if a + b in made or len(a + b) > 24:
            continue
        made.add(a + b)
        merges.append((a, b))
        (right if b.endswith("</w>") else left).append(a + b)
        if not b.endswith("</w>"):
            right.append(a + b)
    return merges


def trained_table(seed=0, n=2000):
    rng = np.random.RandomState(seed)
    corpus = NAMES + WORDS + [w + s for w in NAMES + WORDS[:60] for s in ("s", "ing", "ed")] + ["'s", "'t", "'re", "'ve", "'m", "'ll", "'d",
                                                                                             "!!!", "...", "?!", "--", ",", "."]
    merges = train_bpe(corpus, n * 3 // 5)
    symbols = [chr(c) for c in range(ord("a"), ord("z") + 1)] + [chr(c) for c in range(ord("0"), ord("9") + 1)] + list("!?.,'-:;\"()")
    return random_merges(rng, symbols, n - len(merges), merges)


def english(rng, n):
    out = []
    punct = ["", "", "", ".", ",", "!", "?", "!!!", " ...", "...ok", " - ", ";"]
    for _ in range(n):
        words = []
        for _ in range(rng.randint(1, 16)):
            r = rng.rand()
            w = NAMES[rng.randint(len(NAMES))] if r < 0.3 else WORDS[rng.randint(len(WORDS))] if r < 0.9 else str(rng.randint(0, 100000))
            if rng.rand() < 0.15:
                w = w.capitalize() if rng.rand() < 0.7 else w.upper()
            if rng.rand() < 0.12:
                w += ["'s", "'t", "'re", "'ve", "'m", "'ll", "'d", "'LL", "'S", "'x", "'"][rng.randint(11)]
            words.append(w + punct[rng.randint(len(punct))])
        seps = [" ", " ", " ", "  ", "\t", "\n", " \r\n", "\x0b", "\x0c"]
        out.append("".join(w + seps[rng.randint(len(seps))] for w in words))
    return out


FIXED_A = ["it's", "'ll 'LL x'd", "don't!!! ...ok", "Fred's dinosaur", "they're we've i'm she'll he'd", "x'sabc 's's ''s !'s '", "'", "''",
           "a1b22c333", "1234567890", "3.14 -7 1,000", "tab\tnew\nline\r\nend   ", "   lead", "trail \t\n", "\x1c\x1d\x1e\x1f between",
           "UPPER lower MiXeD", "don'T WON'T 'RE 'Ve", "pororo and loopy are walking in the snow.", "fred , wilma and barney ."]


def set_a(rng):
    return FIXED_A + english(rng, 300 - len(FIXED_A))


OUT_OF_ORDER = [("ab", "a"), ("a", "b"), ("ab", "ab</w>"), ("a", "b</w>")]
REPEATED = [("a", "a"), ("a", "a</w>"), ("aa", "a</w>")]


def set_b():
    t = []
    for k in range(1, 13):
        t += ["a" * k, "ab" * k, "ab" * k + "a", "a" * k + " " + "ab" * k, "b" + "a" * k]
    return t


def set_c(rng, n=200):
    out = []
    for _ in range(n):
        out.append(" ".join("".join("abcd"[rng.randint(4)] for _ in range(rng.randint(1, 14))) for _ in range(rng.randint(1, 6))))
    return out


ADDED = ["fred", "pororo", "loopy", "Eddy", "crong", "fredd", "wil", "x-ray", "b2"]      # "fred" is a prefix of "fredd"


def set_d(rng):
    t = ["fredfred Fred's dinosaur", "alfred", "FRED", "fredd", "freddy fredd fre fred", "fredx xfred xfredx", "afredd", "wilma wil will w il",
         "pororoloopy", "PORORO's", "eddy Eddy EDDY eddying", "x-ray x-rays X-RAY x - ray xx-ray", "b2 b22 ab2 b 2", "crong!crong?crong",
         "<|startoftext|>", "<|endoftext|>", "a<|endoftext|>b", "fred<|endoftext|>fred <|startoftext|>loopy", "<|ENDOFTEXT|>", "<|endoftext|",
         "<|endoftext|><|endoftext|>", "<|startoftext|> hi <|endoftext|> pororo", "fre<|endoftext|>d", "", " ", "fred", "fred fred fred fred"]
    base = english(rng, 120)
    return t + base + [s.replace(" ", "", 2) for s in base[:60]]


def set_e(rng, cap):
    letters = lambda k: "".join(chr(97 + rng.randint(26)) for _ in range(k))
    t = ["", " ", "\t\n", bytes(range(128)).decode("ascii"), bytes(range(127, -1, -1)).decode("ascii"), letters(63), letters(64), letters(65),
         letters(200), "a" * 200, letters(63) + " " + letters(65), "!" * 130, "7" * 95, ("ab " * (cap // 3 + 1))[:cap], letters(cap),
         (letters(3) + " ") * 22, "x " * 1 + "y", "x y z", "x y z w"]
    # rows that fill max_length exactly and by one more, for each max_length: k single-digit words are k tokens
    for L in (5, 77, 85, 91):
        for k in (L - 3, L - 2, L - 1, L):
            t.append(" ".join("0123456789"[i % 10] for i in range(k)))
    return t + english(rng, 40)


def hf_run(merges, added, texts, max_lengths):
    from transformers import CLIPTokenizer
    vocab = O.make_vocab(merges)
    tok = CLIPTokenizer(vocab=vocab, merges=[tuple(m) for m in merges])
    n_new = tok.add_tokens(list(added)) if added else 0
    out = {"lengths": np.array([len(r) for r in tok(texts)["input_ids"]], dtype=np.int32), "n_new": n_new, "size": len(tok)}
    for L in max_lengths:
        enc = tok(texts, padding="max_length", max_length=L, truncation=True, return_tensors="np")
        out[f"ids_{L}"], out[f"mask_{L}"] = enc["input_ids"].astype(np.int64), enc["attention_mask"].astype(np.int64)
    return vocab, out


def mint(path, merges, added, texts, max_lengths):
    vocab, hf = hf_run(merges, added, texts, max_lengths)
    orc = O.Oracle(vocab, merges)
    n_new = orc.add_tokens(added)
    assert (n_new, len(orc)) == (hf["n_new"], hf["size"]), f"add_tokens: oracle {(n_new, len(orc))}, transformers {(hf['n_new'], hf['size'])}"
    for L in max_lengths:
        got = orc(texts, max_length=L, truncation=True)
        for key, want in (("input_ids", hf[f"ids_{L}"]), ("attention_mask", hf[f"mask_{L}"]), ("lengths", hf["lengths"])):
            bad = np.nonzero((got[key] != want).reshape(len(texts), -1).any(axis=1))[0]
            if len(bad):
                r = int(bad[0])
                raise SystemExit(f"{path}: the oracle differs from transformers in {key} of {len(bad)} captions (max_length {L}), first "
                                 f"{texts[r]!r}:\n  oracle       {got[key][r].tolist()}\n  transformers {want[r].tolist()}\nnothing written")
    raw = [t.encode("ascii") for t in texts]
    data = dict(tokens=np.array(sorted(vocab, key=vocab.get)), merges=np.array([f"{a} {b}" for a, b in merges]),
                added=np.array(list(added), dtype=str), text=np.frombuffer(b"".join(raw), dtype=np.uint8),
                offsets=np.cumsum([0] + [len(r) for r in raw]).astype(np.int32), max_lengths=np.array(max_lengths, dtype=np.int32),
                lengths=hf["lengths"])
    for L in max_lengths:
        data[f"ids_{L}"], data[f"mask_{L}"] = hf[f"ids_{L}"], hf[f"mask_{L}"]
    np.savez_compressed(path, **data)
    print(f"{path}: {len(texts)} captions, {len(merges)} merges, {len(added)} added, longest {int(hf['lengths'].max())} tokens, "
          f"{os.path.getsize(path)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--cap", type=int, default=1024, help="the caption byte cap (RCDM_TOK_MAX_CAPTION)")
    a = ap.parse_args()
    rng = np.random.RandomState(20260101)
    table = trained_table()
    p = lambda name: os.path.join(a.out, f"tok_{name}.npz")
    mint(p("english"), table, [], set_a(rng), [85, 77])
    mint(p("out_of_order"), OUT_OF_ORDER, [], set_b(), [77])
    mint(p("repeated"), REPEATED, [], set_b(), [77])
    for k in (0, 1):
        mint(p(f"random{k}"), random_merges(np.random.RandomState(100 + k), list("abcd"), 24 + 16 * k), [], set_c(rng), [77])
    mint(p("added"), table, ADDED, set_d(rng), [85, 77])
    mint(p("shapes"), table, [], set_e(rng, a.cap), [5, 77, 85, 91])


if __name__ == "__main__":
    main()
