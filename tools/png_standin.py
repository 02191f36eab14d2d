#!/usr/bin/env python
"""png_match_block_kernel without a GPU: csrc/png.hip compiled for the CPU behind tools/png_standin/common.h (every lane of a
workgroup a thread, barriers as barriers, LDS as shared statics, atomics as atomics) as a stand-alone program under ASan +
UBSan, run on the filtered stream of every image of the pngm_* goldens; its file must equal the golden byte for byte.
Checks the algorithm and the indexing (an out-of-range LDS or workspace index is a sanitizer report), not the gfx950 code
object.  The filter kernel is not run (the stream comes from tests/png_oracle.py).  Needs g++; about ten seconds an image.

    python tools/png_standin.py [golden names ...]"""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import png_oracle as P  # noqa: E402


def main():
    names = sys.argv[1:] or sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "pngm_*.npz")))
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(os.path.join(ROOT, "rcdms_amd", "csrc", "png.hip"), tmp)
        for f in ("common.h", "main.cpp"):
            shutil.copy(os.path.join(ROOT, "tools", "png_standin", f), tmp)
        exe = os.path.join(tmp, "main")
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-pthread", "-I", tmp, "-I", os.path.join(ROOT, "include"),
                               os.path.join(tmp, "main.cpp"), "-o", exe])
        bad = 0
        for name in names:
            g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
            filt = json.loads(str(g["meta"]))["filter"]
            ends = np.cumsum(g["sizes"])
            for k, img in enumerate(g["input"]):
                want = g["files"][ends[k] - g["sizes"][k]:ends[k]].tobytes()
                h, w, _ = img.shape
                stream, out = os.path.join(tmp, "stream.bin"), os.path.join(tmp, "out.png")
                P.filter_stream(img, filt)[0].tofile(stream)
                r = subprocess.run([exe, str(h), str(w), stream, out], capture_output=True, text=True)
                ok = r.returncode == 0 and open(out, "rb").read() == want
                bad += not ok
                print(f"{name}[{k}]: {'equal' if ok else 'DIFFERENT'} (exit {r.returncode}) {r.stdout.strip()}", flush=True)
                if r.returncode:
                    print(r.stderr[-3000:])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
