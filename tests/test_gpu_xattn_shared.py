"""-m gpu: K3s (soc_xattn_shared_q_f32, include/soc_hip_xattn_shared.h) -- one set of query rows, E expressions -- against
K3 called once per expression and against the CPU oracle, plus its memory contract.  C = 256, 8 heads, fp32."""
import pytest
import torch

from oracle import soc_oracle as O
from tests import guarded

pytestmark = pytest.mark.gpu

C, HEADS = 256, 8
TOL = 2e-5                     # the bound test_mha_core_vs_oracle applies to K3

# Lq, Lk, E, pads per expression (None: no mask at all)
CASES = [(1, 1, 1, None),                      # smallest case
         (63, 1, 2, None),                     # part wave
         (65, 13, 3, (0, 4, 12)),              # wave boundary; a pad count per expression
         (257, 64, 2, None),                   # workgroup boundary, LDS limit
         (700, 17, 5, (0, 1, 2, 3, 4))]        # several workgroups


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from neurips2023_soc_amd import _lib, hot_ops, xattn_shared
    return hot_ops, xattn_shared, _lib


def make(Lq, Lk, E, pads, seed=None):
    g = torch.Generator().manual_seed(Lq * 7 + Lk * 3 + E if seed is None else seed)
    q = torch.randn(Lq, C, generator=g)
    k, v = torch.randn(E, Lk, C, generator=g), torch.randn(E, Lk, C, generator=g)
    kpm = None
    if pads is not None:
        kpm = torch.zeros(E, Lk, dtype=torch.bool)
        for e, p in enumerate(pads):
            assert p < Lk                       # every expression keeps at least one unpadded key
            if p:
                kpm[e, Lk - p:] = True
    return q, k, v, kpm


def k3_per_expression(ops, q, k, v, kpm):
    return torch.stack([ops.mha_core(q[None], k[e:e + 1], v[e:e + 1], HEADS, None if kpm is None else kpm[e:e + 1],
                                     batch_first=True)[0] for e in range(k.shape[0])])


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.mark.parametrize("Lq,Lk,E,pads", CASES)
def test_shared_q_vs_k3_and_oracle(mods, Lq, Lk, E, pads):
    ops, xs, _ = mods
    q, k, v, kpm = make(Lq, Lk, E, pads)
    dq, dk, dv, dm = q.cuda(), k.cuda(), v.cuda(), None if kpm is None else kpm.cuda()
    before = xs.fallbacks
    out = xs.mha_core_shared_q(dq, dk, dv, HEADS, dm)
    assert xs.fallbacks == before, "a supported shape went to K3"
    assert out.shape == (E, Lq, C)
    k3 = k3_per_expression(ops, dq, dk, dv, dm)
    print(f"K3s vs K3: max diff {maxdiff(out, k3):.3e}, bit-equal: {torch.equal(out, k3)}")
    for e in range(E):
        ref = O.mha_core(q[:, None], k[e][:, None], v[e][:, None], HEADS, None if kpm is None else kpm[e:e + 1])[:, 0]
        d_k3, d_or = maxdiff(out[e], k3[e]), maxdiff(out[e], ref)
        print(f"  expression {e}: vs K3 {d_k3:.3e}, vs oracle {d_or:.3e}")
        assert d_k3 < TOL and d_or < TOL, (e, d_k3, d_or)


def test_unsupported_shape_goes_to_k3(mods):
    ops, xs, lib = mods
    q, k, v, kpm = make(70, 65, 2, (0, 3))
    dq, dk, dv, dm = q.cuda(), k.cuda(), v.cuda(), kpm.cuda()
    raw = torch.empty(2, 70, C, device="cuda")
    assert xs.shared_q_raw(dq, dk, dv, dm.to(torch.uint8), raw, HEADS, C // HEADS) == lib.SOC_EUNSUPPORTED
    assert xs.shared_q_raw(dq, dk[:, :64].contiguous(), dv[:, :64].contiguous(), None, raw, 4, 64) == lib.SOC_EUNSUPPORTED
    before = xs.fallbacks
    out = xs.mha_core_shared_q(dq, dk, dv, HEADS, dm)
    assert xs.fallbacks == before + 1
    assert torch.equal(out, k3_per_expression(ops, dq, dk, dv, dm))


def test_invalid_sizes(mods):
    _, xs, lib = mods
    q, k = torch.zeros(4, C, device="cuda"), torch.zeros(1, 3, C, device="cuda")
    out = torch.zeros(1, 4, C, device="cuda")
    assert xs.shared_q_raw(q, k[:0], k[:0], None, out, HEADS, 32) == lib.SOC_EINVAL           # E = 0
    assert xs.shared_q_raw(q[:0], k, k, None, out, HEADS, 32) == lib.SOC_EINVAL               # Lq = 0
    assert xs.shared_q_raw(q, k[:, :0], k[:, :0], None, out, HEADS, 32) == lib.SOC_EINVAL     # Lk = 0
    assert float(out.abs().max()) == 0.0


def test_expressions_are_isolated(mods):
    _, xs, _ = mods
    q, k, v, kpm = make(300, 13, 3, (0, 4, 2))
    dq, dk, dv, dm = q.cuda(), k.cuda(), v.cuda(), kpm.cuda()
    base = xs.mha_core_shared_q(dq, dk, dv, HEADS, dm)
    k2, v2, m2 = dk.clone(), dv.clone(), dm.clone()
    k2[1] += 1.0
    a = xs.mha_core_shared_q(dq, k2, dv, HEADS, dm)
    v2[1] *= -2.0
    b = xs.mha_core_shared_q(dq, dk, v2, HEADS, dm)
    m2[1, :5] = True
    c = xs.mha_core_shared_q(dq, dk, dv, HEADS, m2)
    for name, got in (("k", a), ("v", b), ("mask", c)):
        assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]), name
        assert not torch.equal(got[1], base[1]), name


def test_repeatable(mods):
    _, xs, _ = mods
    q, k, v, kpm = make(700, 17, 5, (0, 1, 2, 3, 4))
    args = (q.cuda(), k.cuda(), v.cuda(), HEADS, kpm.cuda())
    assert torch.equal(xs.mha_core_shared_q(*args), xs.mha_core_shared_q(*args))


@pytest.mark.parametrize("Lq,Lk,E,pads", [(65, 13, 3, (0, 4, 12)), (257, 64, 2, None)])
def test_memory_contract(mods, Lq, Lk, E, pads):
    """`out` inside poisoned guards (at least 256 rows each side): only [E,Lq,C] is written -- row Lq of an odd Lq included --
    every element of it under both patterns, and the inputs are unchanged."""
    ops, xs, _ = mods
    q, k, v, kpm = make(Lq, Lk, E, pads)
    inputs = {"q": q, "k": k, "v": v}
    if kpm is not None:
        inputs["kpm"] = kpm

    def call(a):
        return xs.mha_core_shared_q(a["q"], a["k"], a["v"], HEADS, a.get("kpm"))

    def reference(a):
        return k3_per_expression(ops, a["q"].cuda(), a["k"].cuda(), a["v"].cuda(), a["kpm"].cuda() if "kpm" in a else None).cpu()

    def compare(i, got, want):
        assert maxdiff(got, want) < TOL

    out = guarded.check_contract(inputs, call, torch.device("cuda"), entry=xs.ENTRY, reference=reference, compare=compare)[0]
    assert out.shape == (E, Lq, C)
