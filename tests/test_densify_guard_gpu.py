"""Guard-band runs (tests/guard.py) of the densification strategy's four entry points - v3a_densify_accumulate, v3a_densify_classify,
v3a_densify_apply, v3a_densify_reset_opacity - through the C ABI: every tensor carved out of a poisoned arena, the workspace at
exactly its stated size.  The results are bit-equal to the plain calls of ops, no byte outside the views changes, the inputs keep
their bits, and a workspace one word short is refused.  With offset 4 the pointers miss 16-byte alignment (the harmonics rows then
start on other phases)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import test_densify_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

p = lambda t: C.c_void_p(t.data_ptr())
NAMES = ("means", "scales", "quats", "opacities", "sh")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _clean(parity, tag, outputs, **info):
    torch.cuda.synchronize()
    bad = {n: G.violations(t) for n, t in outputs.items()}
    print(f"[densify guard {tag}] {info}; violations { {n: v[0] for n, v in bad.items()} }")
    parity(f"densify::guard_{tag}", violations=sum(v[0] for v in bad.values()), **info)
    for n, (cnt, where) in bad.items():
        assert cnt == 0, (n, cnt, where)


@pytest.mark.parametrize("U,Cn,offset", [(1, 1, 0), (5, 3, 4), (1027, 1, 4), (1027, 3, 0)])
def test_accumulate(hip_lib, parity, U, Cn, offset):
    from vist3a_amd import ops
    g = np.random.default_rng(U + Cn)
    d = torch.from_numpy((g.normal(size=(Cn, U, 2)) * 1e-4).astype(np.float32)).cuda()
    radii = torch.from_numpy(g.integers(-1, 4, (Cn, U)).astype(np.int32)).cuda()
    grad, count = torch.from_numpy(g.random(U).astype(np.float32)).cuda(), torch.from_numpy(g.integers(0, 5, U).astype(np.int32)).cuda()
    want = (grad.clone(), count.clone())
    ops.densify_accumulate(*want, d, radii, 64, 48)
    g_d, g_r, g_g, g_c = (G.carve_like(x, offset_bytes=offset) for x in (d, radii, grad, count))
    assert hip_lib.v3a_densify_accumulate(p(g_d), p(g_r), U, Cn, 64, 48, p(g_g), p(g_c), _stream()) == 0
    _clean(parity, "accumulate", dict(grad2d=g_g, count=g_c), U=U, C=Cn, offset=offset)
    assert G.unchanged(g_d, d) and G.unchanged(g_r, radii)
    assert torch.equal(G.bits(g_g), G.bits(want[0])) and torch.equal(g_c, want[1])


@pytest.mark.parametrize("U,K,offset", [(1, 1, 0), (5, 4, 4), (1027, 25, 0), (1027, 25, 4), (70_001, 1, 4)])
def test_classify_and_apply(hip_lib, parity, U, K, offset):
    from vist3a_amd import lib, ops
    L = hip_lib
    grad, count, ps, ms, vs = T.scene(U, K)
    tg, tc = torch.from_numpy(grad).cuda(), torch.from_numpy(count).cuda()
    tight = [T.to_gpu(ps), T.to_gpu(ms), T.to_gpu(vs)]
    cls = T.gpu_classify(grad, count, ps, prune_big=True, revised=True)
    new = ops.densify_apply(cls, *tight, seed=5, step=9, revised_opacity=True)
    need = int(L.v3a_densify_classify_workspace_bytes(U))
    assert need == ((3 * ((U + 255) // 256) * 4 + 7) // 8) * 8
    g_grad, g_count = G.carve_like(tg, offset_bytes=offset), G.carve_like(tc, offset_bytes=offset)
    old = [{k: G.carve_like(x, offset_bytes=offset) for k, x in d.items()} for d in tight]
    g_fates = G.carve_like(torch.full((U,), 9, dtype=torch.uint8, device="cuda"), offset_bytes=offset)
    g_counts = G.carve_like(torch.full((3, U), 7, dtype=torch.int32, device="cuda"), offset_bytes=offset)
    g_offsets = G.carve_like(torch.full((3, U), 7, dtype=torch.int32, device="cuda"), offset_bytes=offset)
    g_totals = G.carve_like(torch.full((3,), 7, dtype=torch.int64, device="cuda"))
    g_ws = G.carve((need // 8,), torch.float64, device="cuda")
    a = lib.DensifyClassifyArgs(p(g_grad), p(g_count), p(old[0]["scales"]), p(old[0]["opacities"]), U, *(T.TH[k] for k in ("grow_grad2d", "grow_scale3d", "prune_opa", "prune_scale3d")),
                                1, 1, 1, p(g_fates), p(g_counts), p(g_offsets), p(g_totals), p(g_ws), need - 8)
    assert L.v3a_densify_classify(C.byref(a), _stream()) == -4                                           # held to its stated size
    a.workspace_bytes = need
    assert L.v3a_densify_classify(C.byref(a), _stream()) == 0
    _clean(parity, "classify", dict(fates=g_fates, counts=g_counts, offsets=g_offsets, totals=g_totals, workspace=g_ws), U=U, offset=offset,
           workspace_bytes=need)
    assert G.unchanged(g_grad, tg) and G.unchanged(g_count, tc)
    assert all(torch.equal(x, cls[k]) for k, x in (("fates", g_fates), ("counts", g_counts), ("offsets", g_offsets), ("totals", g_totals)))
    U_out = new[0]["means"].shape[0]
    assert U_out > 0
    out = [{k: G.carve_like(torch.full_like(x, 3.0), offset_bytes=offset) for k, x in d.items()} for d in new]   # every element must be WRITTEN
    b = lib.DensifyApplyArgs(*(p(d[k]) for d in old + out for k in NAMES), p(g_fates), p(g_offsets), p(g_totals), U, U_out, K, 5, 9, 1)
    assert L.v3a_densify_apply(C.byref(b), _stream()) == 0
    _clean(parity, "apply", {f"{g}.{k}": d[k] for g, d in zip(("params", "m", "v"), out) for k in NAMES}, U=U, K=K, U_out=U_out, offset=offset)
    for d, t in zip(old, tight):
        assert all(G.unchanged(d[k], t[k]) for k in NAMES)
    for d, t in zip(out, new):
        for k in NAMES:
            assert torch.equal(G.bits(d[k]), G.bits(t[k])), k
    b.new_sh = b.sh                                                                                       # old and new alias: refused
    assert L.v3a_densify_apply(C.byref(b), _stream()) == -2


@pytest.mark.parametrize("U,offset", [(1, 0), (5, 4), (1027, 4)])
def test_reset_opacity(hip_lib, parity, U, offset):
    from vist3a_amd import ops
    g = np.random.default_rng(U)
    lg = torch.from_numpy((g.normal(size=U) * 3).astype(np.float32)).cuda()
    want, m, v = lg.clone(), torch.ones(U, device="cuda"), torch.ones(U, device="cuda")
    ops.densify_reset_opacity(want, m, v, 0.01)
    g_lg, g_m, g_v = (G.carve_like(x, offset_bytes=offset) for x in (lg, torch.ones(U, device="cuda"), torch.ones(U, device="cuda")))
    assert hip_lib.v3a_densify_reset_opacity(p(g_lg), p(g_m), p(g_v), U, 0.01, _stream()) == 0
    _clean(parity, "reset", dict(logits=g_lg, m=g_m, v=g_v), U=U, offset=offset)
    assert torch.equal(G.bits(g_lg), G.bits(want)) and not bool(g_m.any()) and not bool(g_v.any())
