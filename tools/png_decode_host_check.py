#!/usr/bin/env python
"""The PNG reader's shared core (csrc/png_inflate.h) under AddressSanitizer + UBSan, on the CPU: tools/png_decode_host.cpp
built as a stand-alone program with -fsanitize=address,undefined and run over
  - every fixture of the pngd_* goldens, corrupt ones included, and every file of the png_* / pngm_* goldens: the status
    of each must be the golden's;
  - `--mutants` (default 3000) files derived from the small fixtures by flipping or replacing 1..4 bytes of the zlib stream
    (one in ten also cut short), container CRCs made right again: whatever the status, the run must end without a
    sanitizer report, and every seventh mutant's status must equal the restatement's (tests/png_decode_oracle.py).
Host code with its own main: no preload.  Exit status 0 only if all of that holds.

    python tools/png_decode_host_check.py [--mutants 3000] [--seed 5] [--cxx c++]"""
import argparse
import collections
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_decode_oracle as D  # noqa: E402


def run(exe, tmp, files):
    paths = []
    for i, data in enumerate(files):
        paths.append(os.path.join(tmp, f"{i}.png"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    out = []
    for at in range(0, len(paths), 500):
        r = subprocess.run([exe] + paths[at:at + 500], capture_output=True, text=True)
        if r.returncode or r.stderr:
            print(r.stderr[-4000:])
            sys.exit(f"sanitizer report or crash (exit {r.returncode})")
        out += [int(ln.split()[0]) for ln in r.stdout.split("\n")[:-1]]
    assert len(out) == len(files)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutants", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "png_decode_host")
        cmd = [a.cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
               os.path.join(ROOT, "rcdms_amd", "csrc"), os.path.join(ROOT, "tools", "png_decode_host.cpp"), "-o", exe]
        print(" ".join(cmd))
        subprocess.check_call(cmd)
        items = [(n, d, s) for g in D.GOLDENS for n, d, s, _ in D.golden(g)[0]] + [(n, d, 0) for n, d, _ in D.written_goldens()]
        got = run(exe, tmp, [d for _, d, _ in items])
        wrong = [(n, s, g) for (n, _, s), g in zip(items, got) if s != g]
        print(f"fixtures: {len(items)} files, {len(wrong)} with another status than the golden's")
        rng = random.Random(a.seed)
        base = [d for g in ("small", "types", "crafted", "corrupt", "flat") for _, d, _, _ in D.golden(g)[0] if len(d) < 40000]
        mutants = []
        for _ in range(a.mutants):
            d = rng.choice(base)
            z = bytearray(D.zlib_stream(d))
            for _ in range(rng.choice([1, 1, 2, 4])):
                k = rng.randrange(len(z))
                z[k] = z[k] ^ (1 << rng.randrange(8)) if rng.random() < 0.5 else rng.randrange(256)
            if rng.random() < 0.1:
                z = z[:rng.randrange(1, len(z) + 1)]
            mutants.append(D.set_stream(d, bytes(z)))
        got = run(exe, tmp, mutants)
        differ = sum(D.decode(mutants[i])[0] != got[i] for i in range(0, len(mutants), 7))
        hist = collections.Counter(D.STATUS_NAMES[g] for g in got)
        print(f"mutants: {len(mutants)} files, no sanitizer report; statuses {dict(sorted(hist.items()))}")
        print(f"restatement on every 7th: {differ} differ")
        sys.exit(1 if wrong or differ else 0)


if __name__ == "__main__":
    main()
