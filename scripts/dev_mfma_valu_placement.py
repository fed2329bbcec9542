"""int8 MFMA rate of 8 MFMAs + n VALU instructions per wave and trip, four waves per SIMD, by WHERE the VALU work stands:
placement 0 = behind the eight interleaved MFMAs (mips_filter_i8's unit before round 23), placement 1 = two chains of four one
after the other, n / 8 instructions of the other chain's examination behind every MFMA (dev; MI355X).
proqa_microbench_mfma_i8_valu_placed.  The two placements alternate in one process; the spread of a cell is max - min of its
repeated readings.  usage: python scripts/dev_mfma_valu_placement.py [reps=6] [out.json]"""
import ctypes
import json
import sys

import torch

sys.path.insert(0, ".")
from proqa_amd import _lib  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
out = sys.argv[2] if len(sys.argv) > 2 else None
lib = _lib.load()
torch.zeros(1, device="cuda")
v = ctypes.c_double()
st = _lib.current_stream_ptr()
ns = (0, 16, 24, 32)
for n in ns:   # warm-up: code objects, clocks
    for pl in (0, 1):
        _lib.check(lib.proqa_microbench_mfma_i8_valu_placed(8.0, n, pl, st, ctypes.byref(v)))
readings = {(n, pl): [] for n in ns for pl in (0, 1)}
for rep in range(reps):
    for n in ns:
        for pl in (0, 1):
            _lib.check(lib.proqa_microbench_mfma_i8_valu_placed(8.0, n, pl, st, ctypes.byref(v)))
            readings[(n, pl)].append(v.value)
table = []
print(f"{'n_valu':>6} {'placement 0 TOP/s (min..max)':>32} {'placement 1 TOP/s (min..max)':>32} {'1 / 0':>7} {'spread':>7}")
for n in ns:
    r0, r1 = readings[(n, 0)], readings[(n, 1)]
    m0, m1 = sum(r0) / len(r0), sum(r1) / len(r1)
    spread = max(max(r0) - min(r0), max(r1) - min(r1))
    table.append({"n_valu": n, "placement0_tops": r0, "placement1_tops": r1, "mean0": m0, "mean1": m1, "ratio": m1 / m0,
                  "spread_tops": spread, "gain_exceeds_spread": bool(m1 - m0 > spread)})
    print(f"{n:6d} {m0:12.0f} ({min(r0):5.0f}..{max(r0):5.0f}) {m1:18.0f} ({min(r1):5.0f}..{max(r1):5.0f}) {m1 / m0:7.3f} {spread / m0:7.3f}")
if out:
    with open(out, "w") as f:
        json.dump({"what": "proqa_microbench_mfma_i8_valu_placed, 8 ms launches, four waves per SIMD, random operands",
                   "device": torch.cuda.get_device_name(0), "reps": reps, "table": table}, f, indent=1)
