"""CPU: the guarded-allocation helper (tests/guarded.py) catches every kind of violation the GPU memory-contract suite looks
for -- committed here by fake ops written in Python on CPU tensors -- and passes a correct op; and every kernel entry point
of the library is claimed by a case of the contract table, so a new kernel without a contract case fails here."""
import pytest
import torch

from tests import guarded as G


# ------------------------------------------------------------------ the fake ops: y = 2 x + 1 through a workspace
def _outside(t, element):
    """One element of the storage `t` lives in, `element` elements away from t's first (negative: in front of it)."""
    return t.as_strided((1,), (1,), t.storage_offset() + element)


def op_correct(t):
    x = t["x"]
    ws = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    ws.copy_(x.reshape(-1) * 2)
    out.copy_((ws + 1).view(x.shape))
    return out


def op_writes_before_start(t):
    out = op_correct(t)
    _outside(out, -1).fill_(7.0)
    return out


def op_writes_past_end(t):
    out = op_correct(t)
    _outside(out, out.numel()).fill_(7.0)
    return out


def op_overruns_workspace(t):
    x = t["x"]
    ws = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    _outside(ws, ws.numel() + 3).fill_(0.0)
    return op_correct(t)


def op_leaves_last_unwritten(t):
    x = t["x"]
    out = torch.empty_like(x)
    out.view(-1)[:-1] = (x * 2 + 1).view(-1)[:-1]
    return out


def op_reads_uninitialised_workspace(t):
    x = t["x"]
    ws = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    out.copy_(x * 2 + 1 + 0.0 * ws.view(x.shape))          # "masked" by a multiplication, not by a select
    return out


def op_reads_past_input(t):
    x = t["x"]
    out = torch.empty_like(x)
    out.copy_(x * 2 + 1)
    out.view(-1)[-1] += 0.0 * _outside(x, x.numel())[0]    # a halo multiplied by a zero mask
    return out


def op_mutates_input(t):
    out = op_correct(t)
    t["x"].view(-1)[0] += 1.0
    return out


def op_allocates_unguarded(t):
    out = torch.empty(t["x"].shape, dtype=torch.float32, device="cpu", pin_memory=False)     # a form the helper does not serve
    out.copy_(t["x"] * 2 + 1)
    return out


def op_inplace(t):
    t["x"].mul_(2).add_(1)
    return t["x"]


def _inputs():
    return dict(x=torch.arange(15, dtype=torch.float32).view(3, 5) - 4.0, n=3)


def _reference(t):
    return t["x"].double() * 2 + 1


def _compare(i, got, want):
    assert float((got.double() - want).abs().max()) < 1e-6


def _check(op, **kw):
    return G.check_contract(_inputs(), op, "cpu", reference=_reference, compare=_compare, **kw)


def test_correct_op_passes():
    out, = _check(op_correct)
    assert torch.equal(out, _inputs()["x"] * 2 + 1)
    _check(op_inplace, inplace=("x",))


@pytest.mark.parametrize("op,message", [
    (op_writes_before_start, r"front guard: 4 bytes changed, first at interior offset\(s\) \[-4"),
    (op_writes_past_end, r"back guard: 4 bytes changed, first at interior offset\(s\) \[60"),
    (op_overruns_workspace, r"allocation #0 \[empty \(15,\).*back guard: 4 bytes changed, first at interior offset\(s\) \[72"),
    (op_leaves_last_unwritten, r"output 0 differs between the two patterns in 4 bytes \(first at byte 56 of 60\)"),
    (op_reads_uninitialised_workspace, r"output 0 differs between the two patterns"),
    (op_reads_past_input, r"output 0 differs between the two patterns in \d bytes \(first at byte 5[6-9]"),
    (op_mutates_input, r"input x was modified by the call"),
    (op_inplace, r"input x was modified by the call"),
    (op_allocates_unguarded, r"output 0 does not live in a guarded arena"),
], ids=lambda v: v.__name__ if callable(v) else "")
def test_each_violation_is_caught(op, message):
    with pytest.raises(G.ContractViolation, match=message):
        _check(op)


def test_wrong_answer_and_unreached_entry_are_caught():
    with pytest.raises(G.ContractViolation, match="output 0 disagrees with the reference"):
        G.check_contract(_inputs(), op_correct, "cpu", reference=lambda t: t["x"].double() * 2, compare=_compare)
    with pytest.raises(G.ContractViolation, match="entry point soc_add_layernorm_f32 was not called"):
        _check(op_correct, entry="soc_add_layernorm_f32")


# ------------------------------------------------------------------ the pieces
def test_place_keeps_values_alignment_and_guards():
    for dtype in (torch.float32, torch.float64, torch.uint8, torch.bool, torch.int64, torch.int32):
        src = (torch.arange(35).view(5, 7) % 2).to(dtype)
        for pattern in G.PATTERNS:
            view, h = G.place(src, pattern=pattern)
            assert view.dtype == dtype and view.shape == src.shape and torch.equal(view, src) and view.is_contiguous()
            assert h.guard % G.GUARD_UNIT == 0 and h.guard >= G.TILE_ROWS * 7 * src.element_size()
            assert (view.data_ptr() - h.arena.data_ptr()) == h.guard and h.guards_intact()
            assert bool((h.front == pattern).all()) and bool((h.back == pattern).all()) and h.back.numel() == h.guard
    view, h = G.place(torch.zeros(0, 4))
    assert view.shape == (0, 4) and h.nbytes == 0 and h.guards_intact()
    with pytest.raises(ValueError):
        G.place(torch.zeros(4), guard_bytes=100)


def test_patterns_differ_in_every_byte_and_one_is_nan():
    a, b = G.PATTERNS
    assert a != b and 0 <= a < 256 and 0 <= b < 256
    nan32 = torch.full((4,), a, dtype=torch.uint8).view(torch.float32)
    nan64 = torch.full((8,), a, dtype=torch.uint8).view(torch.float64)
    assert bool(torch.isnan(nan32).all()) and bool(torch.isnan(nan64).all())


def test_guarded_allocations_serves_the_forms_hot_ops_uses_and_nothing_else(monkeypatch):
    real = (torch.empty, torch.zeros, torch.empty_like)
    like = torch.ones(3, 4)
    for mp in (None, monkeypatch):
        with G.guarded_allocations("cpu", G.PATTERNS[1], monkeypatch=mp) as served:
            a = torch.empty((2, 3), dtype=torch.float32, device="cpu")
            b = torch.empty(2, 3, 4, dtype=torch.uint8, device=torch.device("cpu"))
            c = torch.empty(like.shape[:-1] + (5,), dtype=torch.int32, device=like.device)
            e = torch.empty_like(like)
            z = torch.zeros(7, dtype=torch.float64, device="cpu")
            n = len(served)
            # not recognised: keywords beyond shape / dtype / device, another device, a non-contiguous empty_like
            p = torch.empty(3, dtype=torch.float32, device="cpu", pin_memory=False)
            m = torch.empty(3, device="meta")
            t_ = torch.empty_like(like.t())
            assert len(served) == n == 5
        assert (torch.empty, torch.zeros, torch.empty_like) == real
        assert [tuple(h.view.shape) for h in served] == [(2, 3), (2, 3, 4), (3, 5), (3, 4), (7,)]
        assert [h.kind for h in served] == ["empty", "empty", "empty", "empty_like", "zeros"]
        assert a.dtype == torch.float32 and c.dtype == torch.int32 and e.dtype == like.dtype and z.dtype == torch.float64
        assert bool((b == G.PATTERNS[1]).all()) and bool((a.view(torch.uint8) == G.PATTERNS[1]).all())      # empty: all pattern
        assert bool((z == 0).all()) and all(h.guards_intact() for h in served)                              # zeros: zero inside
        assert p.shape == (3,) and m.device.type == "meta" and t_.shape == (4, 3)
    with pytest.raises(RuntimeError, match="boom"):
        with G.guarded_allocations("cpu"):
            raise RuntimeError("boom")
    assert (torch.empty, torch.zeros, torch.empty_like) == real                                             # nothing leaks out


def test_recording_proxy_notes_soc_calls_and_restores_the_library():
    from neurips2023_soc_amd import _lib
    real = _lib.load()
    with G.record_lib_calls() as calls:
        assert _lib.load().soc_hip_abi_version() == _lib.ABI_VERSION
        assert _lib.load().soc_mlp_split_max_hidden(256) == 3584
    assert calls == ["soc_hip_abi_version", "soc_mlp_split_max_hidden"] and _lib.load() is real


# ------------------------------------------------------------------ coverage of the C ABI by the contract table
def _launches_a_kernel(name):
    return not (name in ("soc_hip_abi_version", "soc_hip_error_string", "soc_stream_cus")
                or name.endswith(("_bytes", "_plan", "_max_hidden")))


def test_every_kernel_entry_point_has_a_contract_case():
    from neurips2023_soc_amd import _lib
    from tests import test_gpu_memory_contract as T
    claimed = {c.entry for c in T.CASES} | {e for c in T.CASES for e in c.also}
    kernels = [n for n in _lib.EXPORTS if _launches_a_kernel(n)]
    assert len(kernels) == 38
    missing = [n for n in kernels if n not in claimed]
    assert not missing, f"no memory-contract case claims {missing}: add one to tests/test_gpu_memory_contract.py"
    assert not claimed - set(_lib.EXPORTS), claimed - set(_lib.EXPORTS)
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
