"""-m gpu: K6b (soc_upsample_threshold_bits, include/soc_hip_bits.h) against K6, the byte kernel it shares its per-pixel
function with -- every comparison here is exact -- its memory contract, its argument checks, and the packed path of the engine and
of the Ref-YouTube-VOS driver down to the bytes of the PNG files."""
import os

import pytest
import torch

from neurips2023_soc_amd import _lib
from neurips2023_soc_amd import packed_masks as PM
from tests import guarded as G

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 63), (2, 3, 5, 7, 64), (2, 3, 5, 7, 65),
          (3, 9, 16, 20, 129),          # up-sampling, odd ratios
          (2, 12, 20, 5, 9),            # down-sampling
          (1, 1, 8, 4, 70),             # h = 1: both row taps are the same row
          (1, 8, 1, 70, 3),             # w = 1
          (0, 4, 4, 8, 8),              # empty
          (2, 90, 160, 720, 1280)]      # the real size


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from neurips2023_soc_amd import hot_ops
    return hot_ops


def logits_of(T, h, w, seed=0):
    return (torch.randn(T, h, w, generator=torch.Generator().manual_seed(1000 * T + 10 * h + w + seed)) * 5).cuda()


def record_of(B, T, h, w, offset, extra, seed=0):
    """[B, R] with each clip's [T,h,w] logits at `offset` of its row, R = offset + T h w + extra, other values around them."""
    R = offset + T * h * w + extra
    rec = (torch.randn(B, R, generator=torch.Generator().manual_seed(77 + seed)) * 5).cuda()
    return rec, R


def raw_call(x_ptr, stride, out_ptr, B, T, h, w, H0, W0, thr=0.0):
    return PM._call(x_ptr, stride, out_ptr, B, T, h, w, H0, W0, thr, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("T,h,w,H0,W0", SHAPES)
def test_bits_equal_the_byte_kernel(ops, T, h, w, H0, W0):
    x = logits_of(T, h, w)
    bits = PM.upsample_threshold_bits(x, (H0, W0))
    assert bits.dtype == torch.uint8 and bits.shape == (T, H0, PM.row_bytes(W0)) and bits.data_ptr() % 8 == 0
    want = ops.upsample_threshold(x, (H0, W0))
    assert torch.equal(PM.unpack(bits, W0), want)
    assert torch.equal(bits, PM.pack(want))                        # ... padding bits included


def test_bits_equal_the_byte_kernel_on_the_threshold(ops):
    """Exact zeros and +-1e-7: values ON the decision boundary.  Both kernels run the same function, so they agree here too."""
    T, h, w, H0, W0 = 2, 9, 16, 40, 129
    g = torch.Generator().manual_seed(5)
    pick = torch.randint(0, 3, (T, h, w), generator=g)
    x = torch.tensor([0.0, 1e-7, -1e-7])[pick].cuda()
    for thr in (1e-7, 0.0):
        bits = PM.upsample_threshold_bits(x, (H0, W0), threshold_logit=thr)
        want = ops.upsample_threshold(x, (H0, W0), threshold_logit=thr)
        assert torch.equal(PM.unpack(bits, W0), want)
    assert 0 < int(want.sum()) < want.numel()


@pytest.mark.parametrize("T,h,w,H0,W0", [(2, 3, 5, 7, 1), (2, 3, 5, 7, 63), (2, 3, 5, 7, 65), (1, 9, 16, 20, 129), (1, 4, 4, 3, 128)])
def test_padding_bits_are_written_as_zero(T, h, w, H0, W0):
    x = torch.full((T, h, w), 3.0).cuda()                           # every pixel set: the data bits are all ones
    RB = PM.row_bytes(W0)
    out = torch.full((T, H0, RB), 0xFF, dtype=torch.uint8, device="cuda")
    assert raw_call(x.data_ptr(), T * h * w, out.data_ptr(), 1, T, h, w, H0, W0) == 0
    every = PM.unpack(out, RB * 8)
    assert bool(every[..., :W0].all()) and not bool(every[..., W0:].any())


def test_group_launch_reads_the_record_in_place():
    B, T, h, w, H0, W0 = 3, 2, 5, 7, 11, 70
    rec, R = record_of(B, T, h, w, offset=1 + 2 * 5, extra=9)
    assert R > T * h * w + 5
    off = 11
    first = rec[0, off:off + T * h * w].view(T, h, w)
    before = PM.launches
    with G.guarded_allocations("cuda") as served:
        got = PM.upsample_threshold_bits(first, (H0, W0), clip_stride=R, clips=B)
    assert PM.launches == before + 1
    assert got.shape == (B, T, H0, PM.row_bytes(W0))
    assert served and all(g.guards_intact() for g in served), [g.violations() for g in served]
    for b in range(B):
        alone = PM.upsample_threshold_bits(rec[b, off:off + T * h * w].view(T, h, w).clone(), (H0, W0))
        assert torch.equal(got[b], alone), b
    # the same through a strided [B,T,h,w] view
    view = rec[:, off:off + T * h * w].view(B, T, h, w)
    assert view.stride(0) == R and torch.equal(PM.upsample_threshold_bits(view, (H0, W0)), got)


def _contract_compare(i, got, want):
    assert got.shape == want.shape and torch.equal(got, want), int((got != want).sum())


def test_memory_contract_single_clip(ops):
    T, h, w, H0, W0 = 2, 3, 5, 7, 65
    inputs = dict(x=logits_of(T, h, w, seed=3).cpu())
    G.check_contract(inputs, lambda t: PM.upsample_threshold_bits(t["x"], (H0, W0)), "cuda", entry=PM.ENTRY,
                     reference=lambda t: PM.pack(ops.upsample_threshold(t["x"].cuda(), (H0, W0))).cpu(), compare=_contract_compare)


def test_memory_contract_group_of_three(ops):
    B, T, h, w, H0, W0, off = 3, 2, 3, 5, 7, 65, 7
    rec, R = record_of(B, T, h, w, offset=off, extra=6, seed=4)
    n = T * h * w

    def call(t):
        return PM.upsample_threshold_bits(t["rec"][0, off:off + n].view(T, h, w), (H0, W0), clip_stride=R, clips=B)

    def reference(t):
        clips = [t["rec"][b, off:off + n].view(T, h, w).cuda().contiguous() for b in range(B)]
        return torch.stack([PM.pack(ops.upsample_threshold(c, (H0, W0))) for c in clips]).cpu()

    G.check_contract(dict(rec=rec.cpu()), call, "cuda", entry=PM.ENTRY, reference=reference, compare=_contract_compare)


def test_argument_checks_return_their_codes_without_a_launch():
    T, h, w, H0, W0 = 2, 3, 5, 7, 65
    x = logits_of(T, h, w).repeat(2, 1, 1)                          # room for B = 2
    out = torch.full((2 * T * H0 * PM.row_bytes(W0) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    n = T * h * w
    before = PM.launches
    assert raw_call(x.data_ptr(), n, out.data_ptr() + 1, 1, T, h, w, H0, W0) == _lib.SOC_EINVAL          # out not 8-byte aligned
    assert raw_call(x.data_ptr(), n, out.data_ptr() + 4, 1, T, h, w, H0, W0) == _lib.SOC_EINVAL
    assert raw_call(x.data_ptr(), n - 1, out.data_ptr(), 2, T, h, w, H0, W0) == _lib.SOC_EINVAL          # clips would overlap
    assert raw_call(x.data_ptr(), 256 * h * w, out.data_ptr(), 256, 256, h, w, H0, W0) == _lib.SOC_EUNSUPPORTED    # B * T = 65536
    assert raw_call(x.data_ptr(), n, out.data_ptr(), 1, T, h, w, 65536, W0) == _lib.SOC_EUNSUPPORTED
    assert raw_call(None, n, out.data_ptr(), 1, T, h, w, H0, W0) == _lib.SOC_EINVAL
    assert raw_call(x.data_ptr(), n, None, 1, T, h, w, H0, W0) == _lib.SOC_EINVAL
    assert raw_call(x.data_ptr(), n, out.data_ptr(), 1, T, 0, w, H0, W0) == _lib.SOC_EINVAL
    assert raw_call(x.data_ptr(), n, out.data_ptr(), -1, T, h, w, H0, W0) == _lib.SOC_EINVAL
    assert raw_call(None, 0, None, 0, T, h, w, H0, W0) == 0 and raw_call(None, 0, None, 3, 0, h, w, H0, W0) == 0   # nothing to do
    assert PM.launches == before + 11                               # (calls of the entry; none of them reached the GPU)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    with pytest.raises(_lib.SocHipError):
        PM.upsample_threshold_bits(x.cpu(), (H0, W0))
    with pytest.raises(_lib.SocHipError):
        PM.upsample_threshold_bits(x.double(), (H0, W0))


# ---------------------------------------------------------------------------------------------------------------------
# engine and driver.  The forward is not bit-repeatable (atomics in library kernels), so nothing here compares two runs: the
# logits each clip's masks were made from are kept, and the files must be what the BYTE path makes of those same logits.

@pytest.fixture(scope="module")
def gpu_model():
    import neurips2023_soc_amd as S
    from neurips2023_soc_amd import weights as W
    model, _, _ = S.build_model(S.default_args(text_encoder_random_init=True))
    W.load_synthetic(model, 2023)
    return model.cuda().eval()


@pytest.mark.parametrize("use_graphs,group", [(False, 1), (True, 2)])
def test_driver_writes_the_files_of_the_byte_path_from_the_same_logits(ops, gpu_model, tmp_path, monkeypatch, use_graphs, group):
    from neurips2023_soc_amd import infer, infer_refytb, png_fast
    from neurips2023_soc_amd import synthetic_dataset as SD
    root = SD.make_dataset(str(tmp_path / "data"), videos=1, frames=3, height=144, width=256, expressions=[3], seed=3)
    kept = {}
    real_unpack = infer.ClipInferencer._unpack
    real_call = infer.ClipInferencer.__call__

    def keep(res, tag):
        assert "masks" not in res and res["masks_packed"].dtype == torch.uint8
        kept[tag[0]] = (res["mask_logits"].clone(), res["mask_size"])

    def unpack_and_keep(self, *args, **kw):
        res = real_unpack(self, *args, **kw)
        keep(res, res["tag"])
        return res

    pending = []

    def call_and_keep(self, clip, ids, orig=None):          # the no-graph path has no tag yet when the result is made
        res = real_call(self, clip, ids, orig)
        pending.append(res)
        return res

    monkeypatch.setattr(infer.ClipInferencer, "_unpack", unpack_and_keep)
    monkeypatch.setattr(infer.ClipInferencer, "__call__", call_and_keep)
    before = PM.launches
    out_dir = str(tmp_path / "out")
    stats = infer_refytb.run(gpu_model, SD.HashTokenizer(), root, out_dir, size=96, max_size=160, decode_workers=2,
                             use_graphs=use_graphs, group=group, packed_masks=True)
    for res in pending:
        keep(res, res["tag"])
    assert stats["expressions"] == 3
    if use_graphs:
        # clips 1 + 2: one full group, ONE launch for both; clip 3: half a group, replayed with a stale slot, one launch
        assert stats["group_replays"] == 2 and stats["stale_slots"] == 1
        assert PM.launches == before + 2
    else:
        assert PM.launches == before + 3
    _, data = infer_refytb.load_meta(root)
    (video, item), = data.items()
    assert len(kept) == 3
    for exp_id in item["expressions"]:
        save_dir = os.path.join(out_dir, video, exp_id)
        logits, size = kept[save_dir]
        assert tuple(size) == (144, 256)
        want = ops.upsample_threshold(logits, size).cpu().numpy()
        for j, name in enumerate(item["frames"]):
            with open(os.path.join(save_dir, name + ".png"), "rb") as f:
                assert f.read() == png_fast.encode(want[j], binarize=True), (exp_id, name)


@pytest.mark.parametrize("sizes,launches", [(((50, 70), (50, 70), (50, 70)), 1), (((50, 70), (33, 129), (50, 70)), 3),
                                            (((50, 70), None, (50, 70)), 2)])
def test_unpack_rows_takes_one_launch_per_group_of_one_size(ops, sizes, launches):
    """ClipInferencer._unpack_rows on a synthetic [n, R] record (no forward): one original size -> one launch from the record,
    anything else -> per clip; either way every clip's bits are what the byte kernel makes of its mask logits."""
    import types
    from neurips2023_soc_amd import infer
    T, H, W, Q = 2, 30, 45, 5
    hm, wm = -(-H // 4), -(-W // 4)
    eng = infer.ClipInferencer(types.SimpleNamespace(num_queries=Q), "cuda", use_graphs=False, group=4, packed_masks=True)
    rec = (torch.randn(4, 1 + T * Q + T * hm * wm, generator=torch.Generator().manual_seed(9)) * 5).cuda()
    before = PM.launches
    out = eng._unpack_rows(rec, (T, H, W, 16), [(f"clip{b}", sz) for b, sz in enumerate(sizes)])
    assert PM.launches == before + launches
    assert [r["tag"] for r in out] == ["clip0", "clip1", "clip2"]
    for b, (r, size) in enumerate(zip(out, sizes)):
        assert torch.equal(r["mask_logits"], rec[b, 1 + T * Q:].view(T, hm, wm)) and "masks" not in r
        if size is None:
            assert "masks_packed" not in r
            continue
        assert r["mask_size"] == size and r["masks_packed"].shape == (T, size[0], PM.row_bytes(size[1]))
        assert torch.equal(PM.unpack(r["masks_packed"], size[1]), ops.upsample_threshold(r["mask_logits"], size))
