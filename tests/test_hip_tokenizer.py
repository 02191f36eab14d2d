"""GPU: rcdm_clip_tokenize / rcdms_amd.tokenizer.ClipTokenizer against every golden (tests/golden/tok_*.npz: transformers'
rows on synthetic vocabularies) — ids, mask, lengths and both pool indices equal element for element, the outputs inside
canary bands (tests/guard.py) — then the consumers: a tiny CLIPTextEncoder fed by the tokenizer against the same encoder fed the
golden ids on the host-checked path (bit-identical), and both pipelines' _encode_prompt against a stub that returns the golden
ids."""
import functools
import types

import numpy as np
import pytest
import torch

from rcdms_amd import clip, hip, synth
from rcdms_amd.tokenizer import ClipTokenizer
from tests import guard
from tests import tokenizer_oracle as O
from tests.test_clip import golden as clip_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(name, L) for name in O.GOLDENS for L in O.golden(name).max_lengths]
KW = dict(padding="max_length", return_tensors="pt")


@functools.lru_cache(maxsize=None)
def tokenizer(name):
    g = O.golden(name)
    tok = ClipTokenizer(g.vocab, g.merges)
    if g.added:
        tok.add_tokens(g.added)
    return tok


def run_guarded(tok, texts, L, truncation, pad_cols=3):
    """One launch into canary-banded outputs (rows above and below, pad_cols columns beside the ids and the mask)."""
    n = len(texts)
    _, ih = guard.guarded_out(n, L, L + pad_cols, torch.int64, device=DEV)
    _, mh = guard.guarded_out(n, L, L + pad_cols, torch.int64, device=DEV)
    _, lh = guard.guarded_out(n, 1, 1, torch.int32, device=DEV)
    _, ph = guard.guarded_out(n, 2, 2, torch.int32, device=DEV)
    offsets, raw = tok.pack_texts(texts)
    tok.launch(offsets, raw, L, truncation, out=(ih.data, mh.data, lh.data, ph.data))
    torch.cuda.synchronize()
    return ih, mh, lh, ph


def assert_rows(handles, g, L, rows):
    ih, mh, lh, ph = handles
    for tag, h, want in (("input_ids", ih, g.ids[L][rows]), ("attention_mask", mh, g.mask[L][rows]),
                         ("lengths", lh, g.lengths[rows][:, None]), ("pool_index", ph, g.pool[L][rows])):
        got = h.data.cpu().numpy()
        bad = np.nonzero((got != want).reshape(len(rows), -1).any(axis=1))[0]
        assert not len(bad), (f"{tag}: {len(bad)} of {len(rows)} captions differ, first {g.texts[rows[bad[0]]]!r}: got "
                              f"{got[bad[0]].tolist()}, want {want[bad[0]].tolist()}")
    for h in handles:                                  # after the values: nothing outside the rows and columns was written
        guard.check_out(h)


@pytest.mark.parametrize("name,L", CASES)
def test_every_golden(name, L):
    g = O.golden(name)
    tok = tokenizer(name)
    rows = list(range(len(g.texts)))
    assert_rows(run_guarded(tok, g.texts, L, True), g, L, rows)
    fit = O.fits(g, L)                                 # truncation off wherever the caption fits: the same rows
    assert_rows(run_guarded(tok, [g.texts[r] for r in fit], L, False, pad_cols=0), g, L, fit)


@pytest.mark.parametrize("n", [1, 5, 257])
def test_batch_sizes(n):
    g = O.golden("english")
    rows = list(range(7, 7 + n))
    assert_rows(run_guarded(tokenizer("english"), [g.texts[r] for r in rows], 77, True), g, 77, rows)


def test_call_returns_device_tensors_and_a_second_call_after_add_tokens():
    g, ga = O.golden("english"), O.golden("added")
    assert g.vocab == ga.vocab and g.merges == ga.merges
    tok = ClipTokenizer(g.vocab, g.merges, model_max_length=85)
    out = tok(g.texts, truncation=True, **KW)                         # max_length from model_max_length
    for k, dt, shape in (("input_ids", torch.int64, (300, 85)), ("attention_mask", torch.int64, (300, 85)),
                         ("lengths", torch.int32, (300,)), ("pool_index", torch.int32, (300, 2))):
        assert out[k] is getattr(out, k) and out[k].is_cuda and out[k].dtype == dt and tuple(out[k].shape) == shape, k
    assert np.array_equal(out.input_ids.cpu().numpy(), g.ids[85]) and np.array_equal(out.pool_index.cpu().numpy(), g.pool[85])
    one = tok("pororo and loopy are walking in the snow.", max_length=77, truncation=False, **KW)      # a str is one caption
    assert np.array_equal(one.input_ids.cpu().numpy(), g.ids[77][[g.texts.index("pororo and loopy are walking in the snow.")]])
    tables = tok._dev[next(iter(tok._dev))][1]
    assert tok.add_tokens(ga.added) == len(ga.added)
    out = tok(ga.texts, max_length=77, truncation=True, **KW)
    assert tok._dev[next(iter(tok._dev))][1] is not tables             # rebuilt by add_tokens, and only then
    for k, want in (("input_ids", ga.ids[77]), ("attention_mask", ga.mask[77]), ("lengths", ga.lengths), ("pool_index", ga.pool[77])):
        assert np.array_equal(out[k].cpu().numpy(), want), k
    tables = tok._dev[next(iter(tok._dev))][1]
    tok(ga.texts[:3], max_length=77, truncation=True, **KW)
    assert tok._dev[next(iter(tok._dev))][1] is tables


def test_overflow_raises_with_truncation_off():
    g = O.golden("shapes")
    tok = tokenizer("shapes")
    first = next(r for r in range(len(g.texts)) if g.lengths[r] > 77)
    with pytest.raises(ValueError, match=f"caption {first} .* is {int(g.lengths[first])} tokens with both specials, max_length is 77"):
        tok(g.texts, max_length=77, truncation=False, **KW)
    exact = [t for t, n in zip(g.texts, g.lengths) if n == 77]          # a row that fills max_length exactly passes
    assert exact and tok(exact, max_length=77, truncation=False, **KW).lengths.cpu().tolist() == [77] * len(exact)


def test_kernel_refuses_what_the_host_checks_would():
    """The kernel's own guard (the C entry takes device offsets and bytes and cannot look): a byte >= 0x80, a caption over the
    cap and offsets out of order each give lengths -1 and the row of the empty caption; their neighbours come out right."""
    g = O.golden("english")
    tok = tokenizer("english")
    L = 77
    good = g.texts[20].encode()
    parts = [good, b"caf\xc3\xa9", good, b"a" * (hip.TOK_MAX_CAPTION + 1), good]
    text = np.frombuffer(b"".join(parts), dtype=np.uint8)
    offsets = np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)
    out = tok.launch(offsets, text, L, True)
    empty = np.array(O.Oracle(g.vocab, g.merges)([""], L, True)["input_ids"][0])
    ids = out.input_ids.cpu().numpy()
    assert out.lengths.cpu().tolist() == [int(g.lengths[20]), -1, int(g.lengths[20]), -1, int(g.lengths[20])]
    for r in (0, 2, 4):
        assert np.array_equal(ids[r], g.ids[L][20])
    for r in (1, 3):
        assert np.array_equal(ids[r], empty)
    offsets = np.array([0, len(good), 3, len(good)], dtype=np.int32)    # caption 1 ends before it starts
    out = tok.launch(offsets, np.frombuffer(good, dtype=np.uint8), L, True)
    assert out.lengths.cpu().tolist()[:2] == [int(g.lengths[20]), -1] and np.array_equal(out.input_ids[1].cpu().numpy(), empty)


# ---- the consumers ----------------------------------------------------------------------------------------------------
VOCAB = 2560            # >= len(tokenizer("added")): the embedding table after the driver's resize_token_embeddings


@functools.lru_cache(maxsize=None)
def encoder(base, eos):
    """The tiny text configuration of tests/test_clip.py with a table that holds the tokenizer's ids and the given eos rule."""
    _, cfg, seed = clip_golden(base)
    cfg = dict(cfg, vocab_size=VOCAB, eos_token_id=eos)
    with torch.device("meta"):
        shapes = {k: v.shape for k, v in clip.CLIPTextEncoder(cfg).state_dict().items()}
    m = clip.CLIPTextEncoder(cfg)
    m.load_state_dict(synth.procedural_state_dict(shapes, seed))
    return m.to(DEV)


def encoders():
    eos = O.golden("added").vocab[O.EOS]
    return [encoder("clip_text_sd", 2), encoder("clip_text_first_eos", eos)]     # the legacy argmax rule, the first-eos rule


def outranking_rows(g, L):
    return [r for r in range(len(g.texts)) if g.pool[L][r, 0] != g.pool[L][r, 1]]


@pytest.mark.parametrize("which", [0, 1])
def test_text_encoder_fed_by_the_tokenizer_is_bit_identical(which):
    g = O.golden("added")
    tok = tokenizer("added")
    assert len(tok) <= VOCAB
    enc = encoders()[which]
    L = 85
    rows = outranking_rows(g, L)[:2] + [0, 1, g.texts.index(""), g.texts.index("a<|endoftext|>b")]
    assert g.ids[L][rows[0]].max() > tok.eos_token_id                         # a row whose added token outranks eos
    want = enc(torch.from_numpy(g.ids[L][rows]).to(DEV))                      # the present path: host range check, host pooling index
    t = tok([g.texts[r] for r in rows], max_length=L, truncation=False, **KW)
    got = enc(t.input_ids, pool_index=t.pool_index, ids_checked=True)
    assert torch.equal(got.last_hidden_state, want.last_hidden_state) and torch.equal(got.text_embeds, want.text_embeds)
    assert torch.equal(got.pooler_output, want.pooler_output)
    if which == 0:     # the two rules pool different rows here: pooling by the other column must differ
        other = enc(t.input_ids, pool_index=t.pool_index.flip(1), ids_checked=True)
        assert not torch.equal(other.text_embeds[:2], want.text_embeds[:2])
    half = enc(t.input_ids, pool_index=t.pool_index)                          # each keyword alone
    assert torch.equal(half.text_embeds, want.text_embeds)
    assert torch.equal(enc(t.input_ids, ids_checked=True).text_embeds, want.text_embeds)
    with pytest.raises(ValueError, match="pool_index"):
        enc(t.input_ids, pool_index=t.pool_index[:, 0])
    with pytest.raises(ValueError, match="vocabulary"):
        enc(torch.full((1, L), VOCAB, device=DEV))                            # without the waiver the range check stands


class _GoldenStub:
    """A tokenizer stub that returns the golden rows (host tensors, as transformers does)."""

    def __init__(self, g):
        self.g, self.calls = g, []

    def __call__(self, texts, padding=None, max_length=None, truncation=None, return_tensors=None):
        rows = [self.g.texts.index(t) for t in texts]
        self.calls.append((max_length, truncation))
        return types.SimpleNamespace(input_ids=torch.from_numpy(self.g.ids[max_length][rows]),
                                     attention_mask=torch.from_numpy(self.g.mask[max_length][rows]))


def captions(g, L):
    rows = outranking_rows(g, L)[:2] + [r for r in range(len(g.texts)) if 5 < g.lengths[r] <= L][:3]
    return [g.texts[r] for r in rows]


def test_stage2_encode_prompt_with_the_tokenizer():
    from rcdms_amd.scheduler import DDIMScheduler
    from src.pipelines.RCDMs_pipeline import RCDMsPipeline
    from tests.test_pipeline_glue import _FakeUNet, _Tag
    g = O.golden("added")
    enc = encoders()[0]
    caps = captions(g, 85)
    out = []
    for tok in (tokenizer("added"), _GoldenStub(g)):
        pipe = RCDMsPipeline(vae=None, text_encoder=enc, tokenizer=tok, unet=_FakeUNet(), local_module=_Tag(1.0), global_module=_Tag(2.0),
                             scheduler=DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear"))
        out.append(pipe._encode_prompt(caps, torch.device(DEV), 1, True, None))
    assert tok.calls == [(85, False), (85, False)]
    assert tuple(out[0].shape) == (10, 85, 768) and torch.equal(out[0], out[1])
    assert not torch.equal(out[0][0], out[0][5])


def test_stage1_encode_prompt_with_the_tokenizer():
    from rcdms_amd.scheduler import UnCLIPScheduler
    from src.pipelines.prior_pipeline import Seq_Inpaint_Prior_Pipeline
    g = O.golden("added")
    enc = encoders()[1]
    caps = captions(g, 85)
    out = []
    for tok in (tokenizer("added"), _GoldenStub(g)):
        pipe = Seq_Inpaint_Prior_Pipeline(prior=None, image_encoder=None, text_encoder=enc, tokenizer=tok, scheduler=UnCLIPScheduler())
        out.append(pipe._encode_prompt(caps, torch.device(DEV), 1, True))
    assert tok.calls == [(85, True), (85, True)]
    for a, b in zip(*out):
        assert torch.equal(a, b)
    emb, hid, mask = out[0]
    assert tuple(emb.shape) == (10, 768) and tuple(hid.shape) == (10, 85, 768) and mask.dtype == torch.bool and mask.is_cuda
    assert mask[:5].sum().item() == 10 and mask[5:].sum().item() == sum(int(g.lengths[g.texts.index(c)]) for c in caps)


def test_a_tokenizer_that_outgrew_the_table_is_refused_by_the_pipeline():
    from rcdms_amd.scheduler import UnCLIPScheduler
    from src.pipelines.prior_pipeline import Seq_Inpaint_Prior_Pipeline
    g = O.golden("added")
    tok = ClipTokenizer(g.vocab, g.merges)
    tok.add_tokens([f"name{i}" for i in range(VOCAB - len(tok) + 1)])
    assert len(tok) == VOCAB + 1
    pipe = Seq_Inpaint_Prior_Pipeline(prior=None, image_encoder=None, text_encoder=encoders()[1], tokenizer=tok,
                                      scheduler=UnCLIPScheduler())
    with pytest.raises(ValueError, match="resize the table"):
        pipe._encode_prompt(["fred"], torch.device(DEV), 1, False)
