"""CPU: the CLIP tokenizer without a device — the pure-Python restatement tests/tokenizer_oracle.py against every golden (ids
minted from transformers' `tokenizers` backend on synthetic vocabularies, tools/mint_tokenizer_golden.py) and against
transformers itself where it imports; the shared core csrc/tokenize_core.h compiled into tools/tokenize_host.cpp and run over
every golden; the argument checks of rcdm_clip_tokenize (nothing is launched: the pointers are never dereferenced); and the
host side of rcdms_amd.tokenizer.ClipTokenizer: file loading, add_tokens, the refusals."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import tokenizer_oracle as O
from tests.test_cabi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2
CASES = [(name, L) for name in O.GOLDENS for L in O.golden(name).max_lengths]


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from rcdms_amd import hip
    return hip, hip.load()


def tokenizer(name, added=True):
    from rcdms_amd.tokenizer import ClipTokenizer
    g = O.golden(name)
    tok = ClipTokenizer(g.vocab, g.merges)
    if added and g.added:
        tok.add_tokens(g.added)
    return tok


# ------------------------------------------------------------------------------------------------ the restatement
def test_goldens_hold_what_the_issue_lists():
    g = O.golden("english")
    assert len(g.merges) == 2000 and len(g.texts) == 300 and g.max_lengths == [85, 77]
    for t in ("it's", "'ll 'LL x'd", "don't!!! ...ok", "tab\tnew\nline\r\nend   "):
        assert t in g.texts
    for name in ("out_of_order", "repeated"):
        assert {"a" * k for k in range(1, 13)} | {"ab" * k for k in range(1, 13)} <= set(O.golden(name).texts)
    g = O.golden("added")
    assert "fred" in g.added and "fredd" in g.added and "fredfred Fred's dinosaur" in g.texts and "a<|endoftext|>b" in g.texts
    g = O.golden("shapes")
    assert g.max_lengths == [5, 77, 85, 91] and "" in g.texts and bytes(range(128)).decode() in g.texts
    words = [w for t in g.texts for w in t.split(" ") if w.isalpha()]
    assert {63, 64, 65, 200} <= {len(w) for w in words} and max(len(t) for t in g.texts) == 1024
    for L in g.max_lengths:        # rows that fill max_length exactly, and by one more
        assert L in g.lengths and L + 1 in g.lengths


@pytest.mark.parametrize("name,L", CASES)
def test_oracle_reproduces_golden(name, L):
    g = O.golden(name)
    orc = O.Oracle(g.vocab, g.merges, g.added)
    got = orc(g.texts, L, True)
    assert np.array_equal(got["input_ids"], g.ids[L]) and np.array_equal(got["attention_mask"], g.mask[L])
    assert np.array_equal(got["lengths"], g.lengths) and np.array_equal(got["pool_index"], g.pool[L])
    rows = O.fits(g, L)
    got = orc([g.texts[r] for r in rows], L, False)
    assert np.array_equal(got["input_ids"], g.ids[L][rows])
    if len(rows) < len(g.texts):
        with pytest.raises(ValueError, match="max_length"):
            orc(g.texts, L, False)


def test_merge_order_is_one_lowest_rank_pair_at_a_time():
    """The backend's order where it differs from 'merge every occurrence of the best pair'."""
    g = O.golden("out_of_order")
    inv = {i: t for t, i in g.vocab.items()}
    toks = lambda orc, s: [inv[i] for i in orc.tokens(s)]
    assert toks(O.Oracle(g.vocab, g.merges), "abab") == ["aba", "b</w>"]
    g = O.golden("repeated")
    inv = {i: t for t, i in g.vocab.items()}
    orc = O.Oracle(g.vocab, g.merges)
    assert toks(orc, "aaaa") == ["aa", "aa</w>"] and toks(orc, "aaaaa") == ["aa", "aaa</w>"]
    assert toks(orc, "aaaaaa") == ["aa", "aa", "aa</w>"]


def test_added_tokens_match_inside_words_and_outrank_eos():
    g = O.golden("added")
    orc = O.Oracle(g.vocab, g.merges, g.added)
    inv = {i: t for t, i in g.vocab.items()}
    fred = dict(orc.added)[b"fred"]
    assert [inv.get(i, i) for i in orc.tokens("alfred")] == ["a", "l</w>", inv.get(fred, fred)] and orc.tokens("FRED") == [fred]
    assert orc.tokens("fredd") == [dict(orc.added)[b"fredd"]]                    # the longer of two that start here
    assert orc.tokens("a<|endoftext|>b")[1] == orc.eos_id and orc.tokens("<|ENDOFTEXT|>") != [orc.eos_id]
    new = [i for _, i in orc.added if i > orc.eos_id]
    assert new and len(orc) == max(new) + 1
    L = 77
    hit = [r for r in range(len(g.texts)) if g.pool[L][r, 0] != g.pool[L][r, 1]]
    assert hit, "no row where an added token outranks eos"
    r = hit[0]
    assert g.ids[L][r, g.pool[L][r, 0]] > orc.eos_id and g.ids[L][r, g.pool[L][r, 1]] == orc.eos_id


@pytest.mark.parametrize("name", ["english", "added", "repeated"])
def test_oracle_equals_transformers(name):
    """Fresh captions (not the goldens') through transformers itself, where it imports."""
    tr = pytest.importorskip("transformers")
    pytest.importorskip("tokenizers")
    g = O.golden(name)
    rng = np.random.RandomState(5)
    alphabet = "abfred ' 19!.\tLOY" if name != "repeated" else "aab "
    texts = ["".join(alphabet[rng.randint(len(alphabet))] for _ in range(rng.randint(0, 40))) for _ in range(150)]
    hf = tr.CLIPTokenizer(vocab=dict(g.vocab), merges=[tuple(m) for m in g.merges])
    if g.added:
        hf.add_tokens(list(g.added))
    want = hf(texts, padding="max_length", max_length=60, truncation=True, return_tensors="np")
    got = O.Oracle(g.vocab, g.merges, g.added)(texts, 60, True)
    assert np.array_equal(got["input_ids"], want["input_ids"]) and np.array_equal(got["attention_mask"], want["attention_mask"])


# ------------------------------------------------------------------------------------------------ the shared core on the CPU
@pytest.fixture(scope="module")
def host_tool(tmp_path_factory):
    """tools/tokenize_host.cpp built with the project's compiler, no sanitizer flags."""
    from rcdms_amd import build
    exe = str(tmp_path_factory.mktemp("tok") / "tokenize_host")
    cmd = [build.HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", build.CSRC, os.path.join(ROOT, "tools", "tokenize_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")
    return exe


@pytest.mark.parametrize("name,L", CASES)
def test_host_tool_on_every_golden(host_tool, tmp_path, name, L):
    g = O.golden(name)
    tok = tokenizer(name)
    path = str(tmp_path / "call.bin")
    tok.dump(path, g.texts, L, True)
    r = subprocess.run([host_tool, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    rows = np.array([[int(v) for v in ln.split()] for ln in r.stdout.decode().splitlines()], dtype=np.int64)
    assert rows.shape == (len(g.texts), 4 + L)
    assert np.array_equal(rows[:, 4:], g.ids[L]) and np.array_equal(rows[:, 0], g.lengths)
    assert np.array_equal(rows[:, 1:3], g.pool[L]) and np.array_equal(rows[:, 3], g.mask[L].sum(axis=1))
    # compare mode, truncation off on the rows that fit
    fit = O.fits(g, L)
    tok.dump(path, [g.texts[i] for i in fit], L, False, expect=g.ids[L][fit])
    r = subprocess.run([host_tool, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().strip() == f"ok {len(fit)} rows", r.stdout.decode()[:2000]


def test_host_tool_reports_a_difference_and_refuses_other_files(host_tool, tmp_path):
    g = O.golden("repeated")
    tok = tokenizer("repeated")
    wrong = g.ids[77][:4].copy()
    wrong[2, 1] += 1
    path = str(tmp_path / "call.bin")
    tok.dump(path, g.texts[:4], 77, True, expect=wrong)
    r = subprocess.run([host_tool, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout.decode().startswith("row 2 differs")
    with open(path, "wb") as f:
        f.write(b"not a call")
    r = subprocess.run([host_tool, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"ClipTokenizer.dump" in r.stderr


# ------------------------------------------------------------------------------------------------ the C-ABI's checks
def test_symbols_declared_exported_and_bound():
    hip, lib = _lib()
    for name in ("rcdm_clip_tokenize", "rcdm_clip_tokenize_workspace_bytes", "rcdm_tok_pair_hash"):
        assert name in declared_symbols() and name in hip.SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(hip.TokenizeDesc) == 48 and ctypes.sizeof(hip.TokAdded) == 48
    text = open(os.path.join(ROOT, "include", "rcdm.h")).read()
    for k, v in (("CAPTION", hip.TOK_MAX_CAPTION), ("ADDED", hip.TOK_MAX_ADDED), ("ROWS", hip.TOK_MAX_ROWS),
                 ("ADDED_LEN", hip.TOK_MAX_ADDED_LEN)):
        assert f"#define RCDM_TOK_MAX_{k} {v} " in text, k
    assert hip.TOK_MAX_RANK == 1 << 22 and "#define RCDM_TOK_MAX_RANK (1 << 22)" in text
    assert hip.TOK_MAX_CAPTIONS == 1 << 20 and "#define RCDM_TOK_MAX_CAPTIONS (1 << 20)" in text
    assert lib.rcdm_version() == 0x000300


def test_pair_hash_and_table_agree_with_the_library():
    hip, lib = _lib()
    from rcdms_amd import tokenizer as T
    rng = np.random.RandomState(0)
    a, b = rng.randint(0, 2 ** 31, size=(2, 200)).astype(np.uint32)
    a[:3], b[:3] = (0, 0xFFFFFFFE, 49407), (0, 0xFFFFFFFF, 49407)
    assert T.pair_hash(a, b).tolist() == [lib.rcdm_tok_pair_hash(int(x), int(y)) for x, y in zip(a, b)]
    g = O.golden("english")
    tok = tokenizer("english")
    table = tok.host_tables()[0]
    slots = table.shape[0]
    assert slots == 4096 and (table[:, 0] != 0xFFFFFFFF).sum() == len(g.merges) <= slots // 2
    for rank in (0, 1, 999, 1999):                     # every entry is found by probing from its hash
        x, y = (g.vocab[t] for t in g.merges[rank])
        at = lib.rcdm_tok_pair_hash(x, y) & (slots - 1)
        while table[at, 0] != 0xFFFFFFFF and (table[at, 0], table[at, 1]) != (x, y):
            at = (at + 1) & (slots - 1)
        assert table[at].tolist() == [x, y, rank, g.vocab[g.merges[rank][0] + g.merges[rank][1]]]


def test_argument_validation_without_gpu():
    """The entry point refuses bad descriptors and buffers before touching the device."""
    hip, lib = _lib()
    n, L = 3, 77
    p = dict(text=0x1000, offsets=0x2000, byte_ids=0x3000, added=0x4000, pairs=0x5000, ids=0x6000, mask=0x7000, lengths=0x8000,
             pool=0x9000)                                                                     # never dereferenced

    def desc(**kw):
        f = dict(ld=L, text_bytes=100, n=n, max_length=L, truncation=1, bos_id=10, eos_id=11, pad_id=11, n_added=2, pair_slots=4096)
        f.update(kw)
        return hip.TokenizeDesc(**f)

    def call(d=None, ws=None, ws_bytes=0, **kw):
        q = dict(p)
        q.update(kw)
        return lib.rcdm_clip_tokenize(ctypes.byref(desc() if d is None else d), q["text"], q["offsets"], q["byte_ids"], q["added"],
                                      q["pairs"], q["ids"], q["mask"], q["lengths"], q["pool"], ws, ws_bytes, None)

    # a caption's symbols live in LDS: no workspace is needed, so RCDM_EWORKSPACE cannot be returned for any size passed
    assert lib.rcdm_clip_tokenize_workspace_bytes(ctypes.byref(desc())) == 0
    assert lib.rcdm_clip_tokenize(None, *p.values(), None, 0, None) == EINVAL
    for k in ("text", "offsets", "byte_ids", "pairs", "ids", "mask", "lengths", "pool"):
        assert call(**{k: None}) == EINVAL, k
    assert call(added=None) == EINVAL                                                     # rows announced, no table
    for bad in (dict(n=0), dict(n=-1), dict(max_length=1), dict(ld=L - 1), dict(bos_id=-1), dict(eos_id=-2), dict(pad_id=-1),
                dict(n_added=-1), dict(text_bytes=-1), dict(pair_slots=0), dict(pair_slots=1), dict(pair_slots=4097),
                dict(pair_slots=6)):
        assert call(desc(**bad)) == EINVAL, bad
    for bad in (dict(n=(1 << 20) + 1), dict(max_length=1027, ld=1027), dict(n_added=67), dict(text_bytes=1 << 31),
                dict(pair_slots=1 << 27)):
        assert call(desc(**bad)) == ESHAPE, bad
    for k in ("ids", "mask"):
        assert call(**{k: 0x6004}) == EINVAL, k                                           # int64 rows
    assert call(pairs=0x5008) == EINVAL                                                   # 16-byte slots
    for k in ("offsets", "byte_ids", "added", "lengths", "pool"):
        assert call(**{k: 0x2002}) == EINVAL, k


# ------------------------------------------------------------------------------------------------ ClipTokenizer's host side
def write_files(d, g, added=None, config=None):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(g.vocab, f, ensure_ascii=False)
    with open(os.path.join(d, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in g.merges) + "\n")
    if added is not None:
        with open(os.path.join(d, "added_tokens.json"), "w") as f:
            json.dump(added, f)
    if config is not None:
        with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
            json.dump(config, f)


def test_file_loading(tmp_path):
    from rcdms_amd.tokenizer import ClipTokenizer
    g = O.golden("added")
    ref = tokenizer("added")
    write_files(str(tmp_path / "plain"), g)
    tok = ClipTokenizer.from_files(str(tmp_path / "plain" / "vocab.json"), str(tmp_path / "plain" / "merges.txt"), model_max_length=85)
    assert len(tok) == len(g.vocab) and tok.model_max_length == 85
    assert (tok.bos_token_id, tok.eos_token_id, tok.pad_token_id) == (g.vocab[O.BOS], g.vocab[O.EOS], g.vocab[O.EOS])
    assert all(np.array_equal(x, y) for x, y in zip(tok.host_tables(), tokenizer("added", added=False).host_tables()))
    ids = dict(ref._added)
    new = {t: ids[t.lower()] for t in g.added if ids[t.lower()] >= len(g.vocab)}          # as written: added_tokens.json keeps the case
    cfg = dict(model_max_length=91, pad_token=dict(content="!", special=True), bos_token=O.BOS, eos_token=dict(content=O.EOS))
    write_files(str(tmp_path / "repo" / "tokenizer"), g, added=dict(new, **{O.BOS: g.vocab[O.BOS]}), config=cfg)
    tok = ClipTokenizer.from_pretrained(str(tmp_path / "repo"), subfolder="tokenizer")
    assert tok.model_max_length == 91 and tok.pad_token_id == g.vocab["!"] and len(tok) == len(g.vocab) + len(new)
    assert sorted(tok._added) == sorted((t.lower(), i) for t, i in new.items())
    write_files(str(tmp_path / "gap"), g, added={"zzz": len(g.vocab) + 3})
    with pytest.raises(ValueError, match="added_tokens.json"):
        ClipTokenizer.from_pretrained(str(tmp_path / "gap"))
    with pytest.raises(FileNotFoundError):
        ClipTokenizer.from_pretrained(str(tmp_path / "absent"))
    with pytest.raises(ValueError, match="byte symbol"):
        ClipTokenizer({O.BOS: 0, O.EOS: 1, "a": 2}, [])
    with pytest.raises(ValueError, match="merges"):
        ClipTokenizer(g.vocab, ["q zzzz"])


def test_add_tokens_count_and_ids():
    g = O.golden("added")
    tok, orc = tokenizer("added", added=False), O.Oracle(g.vocab, g.merges)
    base = len(tok)
    assert base == len(g.vocab) == len(orc)
    assert tok.add_tokens(g.added) == orc.add_tokens(g.added) == len(g.added)      # the backend counts vocabulary entries too
    assert len(tok) == len(orc) and [(k.decode(), i) for k, i in orc.added] == tok._added
    assert [i for _, i in tok._added if i >= base] == list(range(base, len(tok)))
    v = tok._version
    assert tok.add_tokens(["fred", "FRED", O.EOS]) == 0 and tok._version == v and len(tok) == len(orc)
    assert tok.add_tokens("newname") == 1 and tok._added[-1] == ("newname", len(tok) - 1) and tok._version == v + 1
    rows = tok.host_tables()[2]
    assert rows.shape == (2 + len(tok._added), 48) and bytes(rows[0, :15]) == O.BOS.encode() and rows[0, 40] == 1 and rows[2, 40] == 0
    assert bytes(rows[2, :4]) == b"fred" and rows[2, 32:40].view(np.int32).tolist() == [4, tok._added[0][1]]
    for bad in (["a b"], [""], ["x" * 33], ["café"], ["tab\t"]):
        with pytest.raises(ValueError, match="added token"):
            tok.add_tokens(bad)
    with pytest.raises(ValueError, match="at most 64"):
        tok.add_tokens([f"name{i}" for i in range(64)])
    assert tok.add_tokens([f"name{i}" for i in range(64 - len(tok._added))]) > 0 and len(tok._added) == 64


def test_refusals_before_any_launch():
    from rcdms_amd import hip
    tok = tokenizer("english")
    kw = dict(padding="max_length", max_length=77, truncation=True, return_tensors="pt")
    with pytest.raises(ValueError, match="not ASCII"):
        tok(["fine", "café au lait"], **kw)
    with pytest.raises(ValueError, match="caption 1 .*not ASCII"):
        tok(["fine", "naïve"], **kw)
    with pytest.raises(ValueError, match="1025 bytes, the cap is 1024"):
        tok(["a" * 1025], **kw)
    for bad in (dict(padding=True), dict(padding="longest"), dict(padding=None), dict(return_tensors="np"), dict(return_tensors=None)):
        with pytest.raises(ValueError, match="padding|return_tensors"):
            tok(["a"], **dict(kw, **bad))
    for bad in (1, 1027):
        with pytest.raises(ValueError, match="max_length"):
            tok(["a"], **dict(kw, max_length=bad))
    with pytest.raises(ValueError, match="no captions"):
        tok([], **kw)
    with pytest.raises(TypeError):
        tok([b"bytes"], **kw)
    with pytest.raises(hip.RcdmError):
        tok.to("cpu")(["a"], **kw)                                                     # no CPU path, with or without a GPU
    tok.to("cuda")


def test_overflow_is_a_value_error_naming_the_caption():
    """truncation=False: the check applied to the lengths read back from the device, here fed the oracle's."""
    g = O.golden("shapes")
    tok = tokenizer("shapes")
    L = 77
    first = next(r for r in range(len(g.texts)) if g.lengths[r] > L)
    with pytest.raises(ValueError) as e:
        tok.check_lengths(g.texts, g.lengths.tolist(), L)
    assert f"caption {first} " in str(e.value) and f"is {int(g.lengths[first])} tokens" in str(e.value) and "max_length is 77" in str(e.value)
    fit = O.fits(g, L)
    tok.check_lengths([g.texts[r] for r in fit], g.lengths[fit].tolist(), L)              # rows that fill max_length exactly pass
    assert L in g.lengths[fit]


def test_pipelines_pass_the_keywords_only_for_the_pair():
    import torch
    from rcdms_amd import clip
    tok = tokenizer("english")
    with torch.device("meta"):
        enc = clip.CLIPTextEncoder(dict(vocab_size=len(tok), hidden_size=64, num_attention_heads=1, num_hidden_layers=1,
                                        intermediate_size=128, projection_dim=64))
        small = clip.CLIPTextEncoder(dict(vocab_size=len(tok) - 1, hidden_size=64, num_attention_heads=1, num_hidden_layers=1,
                                          intermediate_size=128, projection_dim=64))
    out = clip.ClipOutput(pool_index="P")
    assert clip.tokenizer_keywords(tok, enc, out) == dict(pool_index="P", ids_checked=True)
    assert clip.tokenizer_keywords(object(), enc, out) == {} and clip.tokenizer_keywords(tok, object(), out) == {}
    with pytest.raises(ValueError, match="resize"):
        clip.tokenizer_keywords(tok, small, out)
