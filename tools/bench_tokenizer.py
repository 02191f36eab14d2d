#!/usr/bin/env python
"""The CLIP tokenizer on the HIP path (rcdms_amd/tokenizer.py) on one MI355X, on a synthetic vocabulary at the real size
(49 408 entries: 512 byte symbols, 48 894 random trained-order merges, the two specials; generated from a seed — no real CLIP
vocabulary is used):
  (i)   one story's 10 rows (5 captions + 5 empty) at max_length 85 (truncation off, the stage-2 call) and 77 (truncation on)
  (ii)  11 040 captions in one call, a test set's worth
  (iii) the text encoder's forward fed by the tokenizer, with and without pool_index / ids_checked, on the tiny configuration
        of the tests and on the SD-1.5 configuration (random-init weights)
Host clock around calls that end in a device synchronise, median [min, max] of --windows windows of --calls calls after
--warmup calls; the launch alone from device events around back-to-back launches on resident inputs.  Baseline:
transformers.CLIPTokenizer on the same vocabulary plus the upload of its ids where transformers imports, else the pure-Python
restatement tests/tokenizer_oracle.py plus the upload; the JSON line says which.  No pass / fail threshold.
usage: python tools/bench_tokenizer.py [--windows 5] [--calls 20] [--warmup 5] [--out FILE]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, n_windows, calls, warmup):
    """-> [median, min, max] ms per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def event_ms(fn, calls, warmup):
    """ms per call from device events around `calls` back-to-back calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / calls, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import bench
    from rcdms_amd import clip, hip
    from rcdms_amd.tokenizer import ClipTokenizer
    from tests import tokenizer_oracle as O
    spec = importlib.util.spec_from_file_location("mint_tokenizer_golden", os.path.join(ROOT, "tools", "mint_tokenizer_golden.py"))
    mint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mint)
    assert torch.cuda.is_available(), "bench_tokenizer.py measures on the GPU"
    dev = torch.device("cuda", 0)

    rng = np.random.RandomState(a.seed)
    symbols = [chr(c) for c in range(ord("a"), ord("z") + 1)] + [chr(c) for c in range(ord("0"), ord("9") + 1)] + list("!?.,'-:;\"()")
    t0 = time.perf_counter()
    merges = mint.random_merges(rng, symbols, 48894)
    vocab = O.make_vocab(merges)
    assert len(vocab) == 49408
    tok = ClipTokenizer(vocab, merges, model_max_length=77)
    build_s = time.perf_counter() - t0
    names = ["fred", "wilma", "barney", "betty", "pebbles", "dino", "slate", "bammbamm", "pororo", "loopy", "eddy", "crong"]
    tok.add_tokens(names)
    test_set = mint.english(rng, 11040)
    KW = dict(padding="max_length", return_tensors="pt")
    lens = tok(test_set[:200], max_length=77, truncation=True, **KW).lengths.cpu().tolist()
    story = [t for t, n in zip(test_set, lens) if 20 <= n <= 77][:5] + [""] * 5       # captions that fit both max_lengths untruncated
    assert len(story) == 10
    W = dict(n_windows=a.windows, calls=a.calls, warmup=a.warmup)

    # the baseline: transformers where it imports, else the restatement
    try:
        from transformers import CLIPTokenizer
        hf = CLIPTokenizer(vocab=dict(vocab), merges=[tuple(m) for m in merges])
        hf.add_tokens(names)
        baseline = "transformers.CLIPTokenizer (tokenizers backend) + upload of input_ids"

        def base(texts, L, trunc):
            return hf(texts, padding="max_length", max_length=L, truncation=trunc, return_tensors="pt").input_ids.to(dev)
    except Exception as e:           # not installed, or an incompatible build
        orc = O.Oracle(vocab, merges, names)
        baseline = f"tests/tokenizer_oracle.py (pure Python; transformers did not import: {type(e).__name__}) + upload of input_ids"

        def base(texts, L, trunc):
            return torch.from_numpy(orc(texts, L, trunc)["input_ids"]).to(dev)

    same = bool(torch.equal(tok(test_set, max_length=77, truncation=True, **KW).input_ids, base(test_set, 77, True)))
    rows = {"ids_equal_to_baseline_on_11040": same}
    for tag, texts, L, trunc, calls in (("story_10x85", story, 85, False, a.calls), ("story_10x77", story, 77, True, a.calls),
                                        ("test_set_11040x77", test_set, 77, True, max(1, a.calls // 10))):
        w = dict(W, calls=calls)
        rows[tag] = {"hip_ms": windows(lambda: tok(texts, max_length=L, truncation=trunc, **KW), **w),
                     "baseline_ms": windows(lambda: base(texts, L, trunc), **w)}
        # the launch alone: inputs resident, no upload, no readback
        offsets, raw = tok.pack_texts(texts)
        n = len(texts)
        d_off, d_txt = torch.from_numpy(offsets).to(dev), torch.from_numpy(raw.copy() if raw.size else np.zeros(1, np.uint8)).to(dev)
        tables, (o_pairs, o_bytes, o_rows) = tok._tables(dev)
        ids, mask = (torch.empty(n, L, dtype=torch.int64, device=dev) for _ in range(2))
        lengths, pool = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, 2, dtype=torch.int32, device=dev)
        d = tok.desc(n, L, trunc, int(raw.size))
        p = tables.data_ptr()
        rows[tag]["launch_ms_device_events"] = event_ms(
            lambda: hip.clip_tokenize(d, d_txt.data_ptr(), d_off.data_ptr(), p + o_bytes, p + o_rows, p + o_pairs, ids.data_ptr(),
                                      mask.data_ptr(), lengths.data_ptr(), pool.data_ptr()), calls, a.warmup)

    # (iii) the text encoder fed by the tokenizer
    tiny = dict(clip.TEXT_DEFAULTS, vocab_size=len(tok), num_hidden_layers=2, max_position_embeddings=85)
    sd15 = dict(clip.TEXT_DEFAULTS, vocab_size=len(tok), max_position_embeddings=85)
    for tag, cfg in (("encoder_tiny_2_layers", tiny), ("encoder_sd15", sd15)):
        with torch.device("meta"):
            m = clip.CLIPTextEncoder(cfg)
        m = m.to_empty(device=dev).eval()
        bench.init_weights_(m)
        t = tok(story, max_length=85, truncation=False, **KW)
        rows[tag] = {"forward_host_checked_ms": windows(lambda: m(t.input_ids), **W),
                     "forward_pool_index_ids_checked_ms": windows(lambda: m(t.input_ids, pool_index=t.pool_index, ids_checked=True), **W),
                     "tokenize_and_forward_ms": windows(lambda: (lambda q: m(q.input_ids, pool_index=q.pool_index, ids_checked=True))(
                         tok(story, max_length=85, truncation=True, **KW)), **W),
                     "baseline_tokenize_and_forward_ms": windows(lambda: m(base(story, 85, True)), **W)}
        del m
        torch.cuda.empty_cache()
    line = json.dumps({"metric": "CLIP tokenizer on the HIP path: ms per call, median [min, max]", "unit": "ms", "n_gpus": 1,
                       "windows": a.windows, "calls": a.calls, "warmup": a.warmup, "vocabulary": "synthetic, 49408 entries, seed %d" % a.seed,
                       "added_tokens": len(names), "table_build_s": round(build_s, 2), "baseline": baseline, "rows": rows})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
