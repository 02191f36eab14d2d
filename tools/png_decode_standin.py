#!/usr/bin/env python
"""rcdm_png_decode without a GPU: csrc/png_decode.hip compiled for the CPU behind tools/png_decode_standin/common.h (every
lane of the wave a thread, barriers as barriers, LDS as shared statics, shuffles as an exchange between two barriers) as a
stand-alone program under ASan + UBSan, run on the buffers rcdms_amd.image.png_decode_plan lays out — padded pitch, a gap in
front of every image — for the pngd_* goldens, corrupt files included.  Statuses and pixels must equal the goldens, and every
byte of dst outside the good files' pixels must still hold the fill.  Checks the wave's side of the reader (ring indices,
flushes, Adler-32, the input chunks, the anti-diagonal unfilter) and the indexing — an out-of-range LDS, workspace, source
or destination index is a sanitizer report — not the gfx950 code object.  Needs g++; a few seconds per golden.

    python tools/png_decode_standin.py [golden names ...]      (default: small types flat crafted corrupt)"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rcdms_amd import image as I  # noqa: E402
from tests import png_decode_oracle as D  # noqa: E402

FILL = 0xA5


def main():
    names = sys.argv[1:] or ["small", "types", "flat", "crafted", "corrupt"]
    with tempfile.TemporaryDirectory() as tmp:
        for f in ("png_decode.hip", "png_inflate.h"):
            shutil.copy(os.path.join(ROOT, "rcdms_amd", "csrc", f), tmp)
        shutil.copy(os.path.join(ROOT, "tools", "png_standin", "common.h"), os.path.join(tmp, "standin_base.h"))
        for f in ("common.h", "main.cpp"):
            shutil.copy(os.path.join(ROOT, "tools", "png_decode_standin", f), tmp)
        exe = os.path.join(tmp, "main")
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-pthread", "-I", tmp, "-I", os.path.join(ROOT, "include"),
                               os.path.join(tmp, "main.cpp"), "-o", exe])
        bad = 0
        for name in names:
            items, _ = D.golden(name)
            for order in ("rgb", "bgr"):
                plan = I.png_decode_plan([it[1] for it in items], pitch=lambda w: 3 * w + 13, gap=333)
                paths = [os.path.join(tmp, f) for f in ("records.bin", "idats.bin", "src.bin", "out.bin")]
                for p, b in zip(paths, (bytes(plan.records), bytes(plan.idats), plan.src.tobytes())):
                    with open(p, "wb") as f:
                        f.write(b)
                r = subprocess.run([exe, str(plan.n), str(plan.n_idat), str(I.PNG_ORDERS[order]), *paths[:3], str(plan.dst_bytes), paths[3]],
                                   capture_output=True, text=True)
                ok = r.returncode == 0
                if ok:
                    out = np.fromfile(paths[3], dtype=np.uint8)
                    status, raw = out[:4 * plan.n].view(np.int32), out[4 * plan.n:]
                    keep = np.ones(raw.shape, dtype=bool)
                    for i, (nm, _, st, px) in enumerate(items):
                        rec = plan.records[i]
                        ok &= int(status[i]) == st
                        if st == 0 and status[i] == 0:
                            h, w = px.shape[:2]
                            view = np.lib.stride_tricks.as_strided(raw[rec.dst_offset:], (h, 3 * w), (rec.dst_pitch, 1))
                            want = px if order == "rgb" else px[:, :, ::-1]
                            ok &= np.array_equal(view.reshape(h, w, 3), want)
                            np.lib.stride_tricks.as_strided(keep[rec.dst_offset:], (h, 3 * w), (rec.dst_pitch, 1))[:] = False
                    ok &= not ((raw != FILL) & keep).any()
                bad += not ok
                print(f"{name} ({order}): {'equal' if ok else 'DIFFERENT'} (exit {r.returncode})", flush=True)
                if r.returncode:
                    print(r.stderr[-3000:])
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
