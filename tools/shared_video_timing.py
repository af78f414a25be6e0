"""GPU time per VIDEO of E expressions on identical frames: the shared-video pipeline (one Video-Swin pass, E expression
slots: graph_runner.shared_group_pipeline_class) against the group pipeline of the same slot count fed the same clip E times
(E = 1: the one-clip pipeline).  Headline geometry (Swin-T, T = 8, 360x640, 10 tokens), hip events around a run of replays,
the two pipelines alternating inside one process, medians over the rounds; the spread of the baseline's own rounds is
reported beside the difference.  Staging the static inputs is inside the timed window for both (the shared form stages one
clip and E token rows per video, the group form E clips and E token rows).  The records of the two forms are compared first.

    python tools/shared_video_timing.py [--out profiles/shared_video.json] [--rounds 7] [--videos 12] [--E 1 2 4 8]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import neurips2023_soc_amd as S  # noqa: E402
from neurips2023_soc_amd import graph_runner as G  # noqa: E402
from neurips2023_soc_amd import weights as W  # noqa: E402


def timed_ms(step, videos):
    """ms per call of step() over `videos` calls, hip events around the whole run"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(videos):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / videos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "shared_video.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--videos", type=int, default=12, help="replays per round and pipeline")
    ap.add_argument("--E", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--geometry", type=int, nargs=4, default=[8, 360, 640, 10], metavar=("T", "H", "W", "L"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    T, H, Wd, L = a.geometry
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    W.load_synthetic(model, 2023)
    model = model.cuda().eval()
    clip = W.synthetic_clip(1, T, H, Wd).cuda()
    rows = []
    for E in a.E:
        ids = [W.synthetic_token_ids(1 + e, L).cuda() for e in range(E)]
        shared = G.shared_group_pipeline_class(E)(model, T, H, Wd, L, "cuda")
        base = (G.PipelinedClipGraph if E == 1 else G.group_pipeline_class(E))(model, T, H, Wd, L, "cuda")

        def shared_video():
            shared.stage_video(clip)
            for s in range(E):
                shared.stage_inputs(ids[s], slot=s)
            return shared.replay()

        def base_video():
            for s in range(E):
                base.stage_inputs(clip, ids[s], slot=s)
            return base.replay()

        shared_video()
        base_video()
        got, want = shared.flush()[0].view(E, -1), base.flush()[0].view(E, -1)
        diff = float((got - want).abs().max())
        same_query = bool((got[:, 0] == want[:, 0]).all())
        for _ in range(3):                                   # steady state of both before the first timed round
            shared_video()
            base_video()
        t_shared, t_base = [], []
        for r in range(a.rounds):                            # alternating, and alternating who goes first
            for who in (("s", "b") if r % 2 == 0 else ("b", "s")):
                if who == "s":
                    t_shared.append(timed_ms(shared_video, a.videos))
                else:
                    t_base.append(timed_ms(base_video, a.videos))
        shared.flush()
        base.flush()
        row = {"E": E, "shared_ms_per_video_median": round(statistics.median(t_shared), 4),
               "baseline_ms_per_video_median": round(statistics.median(t_base), 4),
               "shared_rounds_ms": [round(t, 4) for t in t_shared], "baseline_rounds_ms": [round(t, 4) for t in t_base],
               "baseline_spread_ms": round(max(t_base) - min(t_base), 4),
               "saved_ms_per_video": round(statistics.median(t_base) - statistics.median(t_shared), 4),
               "records_max_abs_diff": diff, "same_queries": same_query,
               "baseline": "one-clip pipeline" if E == 1 else f"group pipeline, {E} slots, the clip staged {E} times"}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del shared, base
        gc.collect()
        torch.cuda.empty_cache()
    result = {"what": "GPU ms per video of E expressions on identical frames (hip events, staging included, medians of alternating "
                      "rounds): shared-video pipeline against the launch-group pipeline of the same slot count",
              "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
              "geometry": {"T": T, "H": H, "W": Wd, "L": L, "backbone": "video-swin-t"}, "rounds": a.rounds,
              "videos_per_round": a.videos, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
