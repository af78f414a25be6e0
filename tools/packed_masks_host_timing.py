"""Host cost of one 720p mask PNG from bytes (png_fast.encode, binarize) and from bits (png_fast.encode_bits), one thread,
interleaved calls, medians -- with and without the pack step the bits path needs when the mask is NOT already packed (in the
driver it is: K6b writes the bits).  CPU only.

    python tools/packed_masks_host_timing.py [--calls 300] [--out profiles/packed_masks_host.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_masks_host.json"))
a = ap.parse_args()

import numpy as np  # noqa: E402

from neurips2023_soc_amd import packed_masks as PM  # noqa: E402
from neurips2023_soc_amd import png_fast  # noqa: E402

rng = np.random.default_rng(7)
blocky = np.kron(rng.random((90, 160)) < 0.4, np.ones((8, 8), dtype=bool))          # tests/test_png_fast.py's 720 x 1280 mask
yy, xx = np.mgrid[0:720, 0:1280]
disc = (yy - 360) ** 2 + (xx - 640) ** 2 < 200 ** 2
res = {"calls_each": a.calls, "threads": 1, "unit": "ms per 720x1280 mask, median of interleaved calls", "masks": {}}
for name, mask in (("blocky_8x8", blocky), ("disc_r200", disc)):
    bits = PM.pack(mask)
    assert png_fast.encode_bits(bits, 1280) == png_fast.encode(mask, binarize=True)
    t = {"encode_bytes": [], "encode_bits": [], "pack_then_encode_bits": [], "copy_bytes": [], "copy_bits": []}
    for _ in range(a.calls):
        c0 = time.perf_counter()
        png_fast.encode(mask, binarize=True)
        c1 = time.perf_counter()
        png_fast.encode_bits(bits, 1280)
        c2 = time.perf_counter()
        png_fast.encode_bits(PM.pack(mask), 1280)
        c3 = time.perf_counter()
        mask.copy()                                   # what flush() copies out of the pinned buffer per mask, either way
        c4 = time.perf_counter()
        bits.copy()
        c5 = time.perf_counter()
        for k, v in zip(t, (c1 - c0, c2 - c1, c3 - c2, c4 - c3, c5 - c4)):
            t[k].append(v * 1e3)
    med = {k: round(statistics.median(v), 4) for k, v in t.items()}
    med["png_bytes"] = len(png_fast.encode_bits(bits, 1280))
    med["speedup_encode_bits_over_encode_bytes"] = round(med["encode_bytes"] / med["encode_bits"], 2)
    res["masks"][name] = med
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
