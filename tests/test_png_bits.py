"""The host side of the bit-packed mask path: soc_png_encode_bits (libsoc_host.so) writes, from the bits, the file
soc_png_encode_u8(binarize=1) writes from the bytes -- identity of the bytes is the specification -- and packed_masks.pack /
unpack are the format of include/soc_hip_bits.h.  No GPU."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from neurips2023_soc_amd import packed_masks as PM
from neurips2023_soc_amd import png_fast
from neurips2023_soc_amd import postprocessing as P

SIZES = [(1, 1), (1, 7), (3, 5), (7, 300), (64, 64), (65, 129), (361, 641), (720, 1280)]
KINDS = ["disc_stripes", "zeros", "ones", "noise", "checker", "last_pixel", "repeated_rows"]


def make_mask(kind, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(h * 7919 + w)
    if kind == "disc_stripes":
        return ((yy - h / 2) ** 2 + (xx - w / 2) ** 2 < (min(h, w) / 3 + 1) ** 2) | (xx % 11 == 3) | (yy % 13 == 5)
    if kind == "zeros":
        return np.zeros((h, w), bool)
    if kind == "ones":
        return np.ones((h, w), bool)
    if kind == "noise":
        return rng.random((h, w)) < 0.5
    if kind == "checker":
        return (yy + xx) % 2 == 0
    if kind == "last_pixel":
        m = np.zeros((h, w), bool)
        m[-1, -1] = True
        return m
    if kind == "repeated_rows":          # every odd row equals the row above: whole scanlines of zeros after the filter
        return np.repeat(rng.random(((h + 1) // 2, w)) < 0.3, 2, axis=0)[:h]
    raise KeyError(kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w", SIZES)
def test_bits_encoder_writes_the_bytes_of_the_byte_encoder(h, w, kind):
    mask = make_mask(kind, h, w)
    want = png_fast.encode(mask, binarize=True)
    got = png_fast.encode_bits(PM.pack(mask), w)
    assert got == want


@pytest.mark.parametrize("h,w", [(3, 5), (7, 300), (65, 129), (361, 641)])
def test_identity_with_a_wider_row_stride_and_garbage_in_the_padding(h, w):
    mask = make_mask("disc_stripes", h, w) ^ make_mask("noise", h, w)
    want = png_fast.encode(mask, binarize=True)
    bits = PM.pack(mask)
    rb = PM.row_bytes(w)
    wide = np.full((h, rb + 24), 0xA7, np.uint8)                 # rows 24 bytes further apart, garbage between them
    wide[:, :rb] = bits
    assert png_fast.encode_bits(wide[:, :rb], w) == want
    assert png_fast.encode_bits(wide, w) == want                 # ... also when the garbage counts as part of the row
    dirty = bits.copy()
    pad = np.unpackbits(np.zeros_like(dirty), axis=-1, bitorder="little")
    pad[:, w:] = 1
    dirty |= np.packbits(pad, axis=-1, bitorder="little")        # every bit at x >= w set
    assert dirty.shape == bits.shape and (w % 64 == 0 or not np.array_equal(dirty, bits))
    assert png_fast.encode_bits(dirty, w) == want
    tight = np.ascontiguousarray(bits[:, :-(-w // 8)])           # the smallest legal stride: ceil(w / 8)
    assert png_fast.encode_bits(tight, w) == want


def test_bad_arguments_return_the_documented_codes():
    lib = png_fast.load()
    bits = np.zeros((4, 8), np.uint8)
    big = np.zeros(lib.soc_png_bound(4, 20), np.uint8)
    small = np.zeros(16, np.uint8)
    assert lib.soc_png_encode_bits(None, 4, 20, 8, big.ctypes.data, big.size) == -1
    assert lib.soc_png_encode_bits(bits.ctypes.data, 4, 20, 8, None, big.size) == -1
    assert lib.soc_png_encode_bits(bits.ctypes.data, 4, 20, 2, big.ctypes.data, big.size) == -1       # stride < ceil(20 / 8)
    assert lib.soc_png_encode_bits(bits.ctypes.data, 0, 20, 8, big.ctypes.data, big.size) == -1
    assert lib.soc_png_encode_bits(bits.ctypes.data, 4, 20, 8, small.ctypes.data, small.size) == -2   # capacity
    assert lib.soc_png_encode_bits(bits.ctypes.data, 4, 20, 3, big.ctypes.data, big.size) > 0
    with pytest.raises(ValueError):
        png_fast.encode_bits(np.zeros((4, 2), np.uint8), 20)
    with pytest.raises(ValueError):
        png_fast.encode_bits(np.zeros((4, 8), np.int8), 20)


@pytest.mark.parametrize("shape", [(1, 1), (7, 63), (7, 64), (7, 65), (2, 3, 5, 129), (3, 20, 1280), (0, 8, 8)])
def test_pack_unpack_round_trip_and_numpy_packbits(shape):
    rng = np.random.default_rng(sum(shape))
    mask = rng.random(shape) < 0.5
    W0 = shape[-1]
    bits = PM.pack(mask)
    assert bits.dtype == np.uint8 and bits.shape == shape[:-1] + (PM.row_bytes(W0),) and PM.row_bytes(W0) % 8 == 0
    ref = np.packbits(mask, axis=-1, bitorder="little")
    assert np.array_equal(bits[..., :ref.shape[-1]], ref) and not bits[..., ref.shape[-1]:].any()
    assert np.array_equal(PM.unpack(bits, W0), mask)
    tb = PM.pack(torch.from_numpy(mask))
    assert tb.dtype == torch.uint8 and np.array_equal(tb.numpy(), bits)
    assert torch.equal(PM.unpack(tb, W0), torch.from_numpy(mask))
    dirty = bits.copy()
    if W0 % 8:
        dirty[..., W0 // 8] |= np.uint8((0xFF << (W0 % 8)) & 0xFF)
    dirty[..., -(-W0 // 8):] = 0xFF
    assert np.array_equal(PM.unpack(dirty, W0), mask) and torch.equal(PM.unpack(torch.from_numpy(dirty), W0), torch.from_numpy(mask))


def test_save_bits_writes_a_file_pillow_reads_back(tmp_path):
    from PIL import Image
    mask = make_mask("disc_stripes", 65, 129)
    png_fast.save_bits(str(tmp_path / "m.png"), PM.pack(mask), 129)
    img = Image.open(tmp_path / "m.png")
    assert img.mode == "L" and np.array_equal(np.array(img), mask.astype(np.uint8) * 255)


def test_eight_threads_get_the_same_bytes():
    masks = [make_mask(k, 361, 641) for k in ("disc_stripes", "noise", "repeated_rows", "checker")]
    packed = [PM.pack(m) for m in masks]
    want = [png_fast.encode(m, binarize=True) for m in masks]

    def work(t):
        bad = 0
        for i in range(40):
            j = (t + i) % len(masks)
            bad += png_fast.encode_bits(packed[j], 641) != want[j]
        return bad

    with ThreadPoolExecutor(max_workers=8) as pool:
        assert sum(pool.map(work, range(8))) == 0


@pytest.mark.parametrize("T,h,w,H0,W0", [(2, 3, 5, 7, 65), (1, 9, 16, 20, 129), (2, 12, 20, 5, 9)])
def test_packed_postprocessing_on_cpu_tensors(T, h, w, H0, W0):
    x = torch.randn(T, h, w, generator=torch.Generator().manual_seed(H0 + W0)) * 5
    got = P.upsample_and_threshold_packed(x, (H0, W0))
    assert got.dtype == torch.uint8 and got.shape == (T, H0, PM.row_bytes(W0))
    assert torch.equal(got, PM.pack(P.upsample_and_threshold(x, (H0, W0))))


def test_packed_masks_flag_is_refused_with_the_davis_driver():
    from neurips2023_soc_amd import infer
    with pytest.raises(SystemExit):
        infer.parse_args(["--dataset", "davis", "--root", "x", "--out", "y", "--packed-masks"])
    assert infer.parse_args(["--dataset", "refytb", "--root", "x", "--out", "y", "--packed-masks"]).packed_masks
    assert not infer.parse_args(["--dataset", "refytb", "--root", "x", "--out", "y"]).packed_masks


def test_a_library_without_the_entry_is_reported_as_stale(monkeypatch):
    from neurips2023_soc_amd import _lib

    class Old:
        pass
    monkeypatch.setattr(_lib, "_lib", Old())
    with pytest.raises(_lib.SocHipError, match="stale"):
        PM._entry()
