"""Guard-band runs (tests/guard.py) of the MCMC strategy's three compute entry points - v3a_mcmc_sample, v3a_mcmc_relocate,
v3a_mcmc_noise - through the C ABI: every tensor carved out of a poisoned arena, the workspaces at exactly their stated size.  The
results are bit-equal to the plain calls of ops, no byte outside the views changes, the inputs keep their bits, and a workspace one
word short is refused.  With offset 4 the pointers miss 16-byte alignment (the noise's quaternions then take the scalar path)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import test_mcmc_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

p = lambda t: C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _clean(parity, tag, outputs, **info):
    torch.cuda.synchronize()
    bad = {n: G.violations(t) for n, t in outputs.items()}
    print(f"[mcmc guard {tag}] {info}; violations { {n: v[0] for n, v in bad.items()} }")
    parity(f"mcmc::guard_{tag}", violations=sum(v[0] for v in bad.values()), **info)
    for n, (cnt, where) in bad.items():
        assert cnt == 0, (n, cnt, where)


@pytest.mark.parametrize("U,alive_only,offset", [(5, True, 4), (1025, True, 0), (1025, False, 4), (70_001, True, 0), (70_001, False, 0)])
def test_sample(hip_lib, parity, U, alive_only, offset):
    from vist3a_amd import ops
    L = hip_lib
    w = torch.from_numpy(T.wide_weights(U)).cuda()
    n = T.slots_of(U, alive_only)
    stream = 0 if alive_only else 1
    src, counts = ops.mcmc_sample(w, min_weight=T.MIN_OP, alive_only=alive_only, n_slots=n, seed=7, stream=stream, step=13)
    need = int(L.v3a_mcmc_sample_workspace_bytes(U))
    assert need == (2 * ((U + 1023) // 1024) + 1) * 8
    g_w = G.carve_like(w, offset_bytes=offset)
    g_src = G.carve_like(torch.full((n,), 7, dtype=torch.int32, device="cuda"), offset_bytes=offset)      # -1 is the poison: start from 7
    g_counts = G.carve_like(torch.full((U,), 7, dtype=torch.int32, device="cuda"), offset_bytes=offset)
    g_ws = G.carve((need // 8,), torch.float64, device="cuda")
    call = lambda nbytes: L.v3a_mcmc_sample(p(g_w), U, T.MIN_OP, int(alive_only), n, 7, stream, 13, p(g_src), p(g_counts), p(g_ws), nbytes, _stream())
    assert call(need - 8) == -4                                                                          # held to its stated size
    assert call(need) == 0
    _clean(parity, "sample", dict(src=g_src, counts=g_counts, workspace=g_ws), U=U, alive_only=alive_only, offset=offset, workspace_bytes=need)
    assert G.unchanged(g_w, w)
    assert torch.equal(g_src, src) and torch.equal(g_counts, counts)


@pytest.mark.parametrize("U,K,growth,offset", [(5, 1, False, 4), (1027, 25, False, 0), (5, 25, True, 0), (1027, 1, True, 4)])
def test_relocate(hip_lib, parity, U, K, growth, offset):
    from vist3a_amd import lib, ops
    import mcmc_oracle as MO
    L = hip_lib
    n = (3 if U == 5 else 51) if growth else U
    ps, ms, vs, w = T.relocation_case(U, K)
    src, counts = MO.sample(w, T.MIN_OP, not growth, n, 11, 1 if growth else 0, 5)
    if growth:
        grow = lambda d: {k: np.concatenate([x, np.full((n,) + x.shape[1:], 3.0, np.float32)]) for k, x in d.items()}
        ps, ms, vs = grow(ps), grow(ms), grow(vs)
    src, counts = torch.from_numpy(src).cuda(), torch.from_numpy(counts).cuda()
    tight = [T.to_gpu(ps), T.to_gpu(ms), T.to_gpu(vs)]
    before = [{k: x.clone() for k, x in d.items()} for d in tight]
    ops.mcmc_relocate(src, counts, *tight, dst_offset=U if growth else 0, min_opacity=T.MIN_OP)
    need = int(L.v3a_mcmc_relocate_workspace_bytes(U))
    assert need == 16 * U
    carved = [{k: G.carve_like(x, offset_bytes=offset) for k, x in d.items()} for d in before]
    g_src, g_counts = G.carve_like(src, offset_bytes=offset), G.carve_like(counts, offset_bytes=offset)
    g_ws = G.carve((need // 8,), torch.float64, device="cuda")
    a = lib.McmcRelocateArgs(p(g_src), p(g_counts), *(p(d[k]) for d in carved for k in MO.NAMES), U, n, U if growth else 0, K, T.MIN_OP,
                             p(g_ws), need - 8)
    assert L.v3a_mcmc_relocate(C.byref(a), _stream()) == -4                                               # held to its stated size
    a.workspace_bytes = need
    assert L.v3a_mcmc_relocate(C.byref(a), _stream()) == 0
    outputs = {f"{g}.{k}": d[k] for g, d in zip(("params", "m", "v"), carved) for k in MO.NAMES}
    _clean(parity, "relocate", dict(workspace=g_ws, **outputs), U=U, K=K, growth=growth, offset=offset, workspace_bytes=need)
    assert G.unchanged(g_src, src) and G.unchanged(g_counts, counts)
    for d, t in zip(carved, tight):
        for k in MO.NAMES:
            assert torch.equal(G.bits(d[k]), G.bits(t[k])), k


@pytest.mark.parametrize("U,offset", [(1, 0), (5, 4), (1027, 0), (1027, 4), (70_001, 0)])
def test_noise(hip_lib, parity, U, offset):
    from vist3a_amd import ops
    L = hip_lib
    means, ls, quats, logits = (torch.from_numpy(x).cuda() for x in T.noise_case(U, False))
    want = means.clone()
    ops.mcmc_noise(want, ls, quats, logits, scaler=T.SCALER, seed=9, step=33)
    g_means, g_ls, g_q, g_lg = (G.carve_like(x, offset_bytes=offset) for x in (means, ls, quats, logits))
    assert L.v3a_mcmc_noise(p(g_means), p(g_ls), p(g_q), p(g_lg), U, T.SCALER, 9, 33, _stream()) == 0
    _clean(parity, "noise", dict(means=g_means), U=U, offset=offset)
    assert G.unchanged(g_ls, ls) and G.unchanged(g_q, quats) and G.unchanged(g_lg, logits)
    assert torch.equal(G.bits(g_means), G.bits(want)) and not torch.equal(want, means)                     # the scalar path gives the same bits
