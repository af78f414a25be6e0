"""-m gpu: both dataset drivers with share_video -- all expressions of a video (DAVIS: of a chunk) in one engine call -- write
the files the unshared drivers write and count the same videos / expressions / frames.  Numerical agreement is asserted on
logits in tests/test_gpu_shared_video.py; here a pixel whose logit lies at the decision boundary may differ between the two
runs, a mask that landed under another expression's name may not."""
import os

import numpy as np
import pytest

from neurips2023_soc_amd import synthetic_dataset as SD

pytestmark = pytest.mark.gpu

SIZE, MAX_SIZE = 96, 160          # tests/test_drivers.py
FLIPS = 1e-4                      # share of pixels that may sit on the decision boundary (the bound of tests/test_drivers.py)


@pytest.fixture(scope="module")
def gpu_model():
    import neurips2023_soc_amd as S
    from neurips2023_soc_amd import weights as W
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    W.load_synthetic(model, 2023)
    return model.cuda().eval()


def tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def compare_trees(a, b):
    from PIL import Image
    files = tree(a)
    assert files == tree(b) and files
    total = wrong = 0
    distinct = set()
    for f in files:
        if not f.endswith(".png"):
            continue
        x, y = np.array(Image.open(os.path.join(a, f))), np.array(Image.open(os.path.join(b, f)))
        assert x.shape == y.shape, f
        total += x.size
        wrong += int((x != y).sum())
        distinct.add(x.tobytes())
    print(f"{len(files)} files, {wrong} of {total} pixels differ")
    assert wrong <= FLIPS * total
    assert len(distinct) > 1                  # the expressions give different masks: a swap of two would show
    return files


@pytest.mark.parametrize("use_graphs,packed", [(False, False), (True, False), (True, True)])
def test_refytb_driver_share_video(gpu_model, tmp_path, use_graphs, packed):
    from neurips2023_soc_amd import infer_refytb
    counts = (3, 1, 4)                        # ragged, as the real set
    root = SD.make_dataset(str(tmp_path / "data"), videos=len(counts), frames=3, height=144, width=256, expressions=list(counts), seed=3)
    tok = SD.HashTokenizer()
    kw = dict(size=SIZE, max_size=MAX_SIZE, decode_workers=2, use_graphs=use_graphs, group=4 if use_graphs else 1, packed_masks=packed)
    plain = infer_refytb.run(gpu_model, tok, root, str(tmp_path / "plain"), **kw)
    shared = infer_refytb.run(gpu_model, tok, root, str(tmp_path / "shared"), share_video=True, **kw)
    for k in ("videos", "expressions", "frames"):
        assert shared[k] == plain[k], k
    assert shared["videos"] == len(counts) and shared["expressions"] == sum(counts) and shared["frames"] == 3 * sum(counts)
    assert plain["shared_video_passes"] == 0 and plain["shared_expressions"] == 0
    assert shared["shared_video_passes"] == len(counts) and shared["shared_expressions"] == sum(counts)
    assert shared["cache_misses"] == len(counts)                  # frames decoded once per video
    if use_graphs:
        assert shared["group_replays"] == 0 and shared["stale_slots"] == sum(4 - c for c in counts)
    files = compare_trees(str(tmp_path / "plain"), str(tmp_path / "shared"))
    assert len(files) == 3 * sum(counts)


@pytest.mark.parametrize("use_graphs", [False, True])
def test_davis_driver_share_video(gpu_model, tmp_path, use_graphs):
    from neurips2023_soc_amd import infer_davis
    # 2 videos, 2 objects x 4 annotators = 8 expressions each, one chunk per video
    root = SD.make_dataset(str(tmp_path / "data"), videos=2, frames=3, height=144, width=256, expressions=8, seed=5)
    tok = SD.HashTokenizer()
    kw = dict(size=SIZE, max_size=MAX_SIZE, decode_workers=2, use_graphs=use_graphs, group=8 if use_graphs else 1)
    plain = infer_davis.run(gpu_model, tok, root, str(tmp_path / "plain"), **kw)
    shared = infer_davis.run(gpu_model, tok, root, str(tmp_path / "shared"), share_video=True, **kw)
    for k in ("videos", "expressions", "frames"):
        assert shared[k] == plain[k], k
    assert shared["videos"] == 2 and shared["expressions"] == 16 and shared["frames"] == 48
    assert plain["shared_video_passes"] == 0
    assert shared["shared_video_passes"] == 2 and shared["shared_expressions"] == 16      # one pass per chunk
    files = compare_trees(str(tmp_path / "plain"), str(tmp_path / "shared"))
    assert len(files) == 2 * 4 * 3                                # videos x annotators x frames
    with pytest.raises(ValueError, match="share_video"):
        from neurips2023_soc_amd.infer import ClipInferencer
        infer_davis.run(gpu_model, tok, root, str(tmp_path / "x"), share_video=True, size=SIZE, max_size=MAX_SIZE,
                        engine=ClipInferencer(gpu_model, "cuda", use_graphs=False))
