"""GPU time of scoring one video's expressions: K27b on packed masks against the route without it (unpack every expression to a
one-object label map, one K27 call per expression).  hip events, median of repeats, one device.

    python tools/refytb_eval_timing.py [--out profiles/refytb_eval.json] [--repeats 30]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neurips2023_soc_amd import davis_eval, hot_ops, jf_bits  # noqa: E402
from neurips2023_soc_amd import packed_masks as PM  # noqa: E402
from neurips2023_soc_amd import synthetic_dataset as SD  # noqa: E402


def gpu_ms(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "refytb_eval.json"))
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    T, H, W, objects = 8, 720, 1280, 2
    radius = davis_eval.bound_radius((H, W))
    gt = torch.from_numpy(SD.blob_label_maps(70, T, H, W, objects, void=True)).cuda()
    rows = []
    for E in (1, 8):
        obj = [1 + e % objects for e in range(E)]
        pred = np.stack([SD.blob_label_maps(70, T, H, W, objects, wobble=0.02 + 0.005 * e) == obj[e] for e in range(E)])
        bits = torch.from_numpy(PM.pack(pred)).cuda()
        distinct = sorted(set(obj))
        exp_obj = [distinct.index(o) for o in obj]

        def k27b():
            return jf_bits.jf_counts_bits(gt, distinct, exp_obj, bits, radius)

        def k27_per_expression():
            out = []
            for e in range(E):
                one = torch.where(gt == 255, gt, (gt == obj[e]).to(torch.uint8))
                out.append(hot_ops.davis_jf_counts(one, PM.unpack(bits[e], W).to(torch.uint8), 1, 1, radius, use_void=True,
                                                   pairs=False)[0])
            return torch.stack(out)

        assert torch.equal(k27b(), k27_per_expression())
        new, new_min = gpu_ms(k27b, a.repeats)
        old, old_min = gpu_ms(k27_per_expression, a.repeats)
        rows.append({"E": E, "k27b_ms_median": round(new, 4), "k27b_ms_min": round(new_min, 4),
                     "unpack_and_k27_per_expression_ms_median": round(old, 4),
                     "unpack_and_k27_per_expression_ms_min": round(old_min, 4)})
        print(rows[-1], flush=True)
    result = {"what": "GPU time (hip events) of the six J&F counts of one video, counts equal between the two routes",
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "frame": [H, W], "T": T, "objects": objects, "radius": radius,
              "repeats": a.repeats, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
