"""Guard-band runs (tests/guard.py) of the three entry points of pose optimisation - v3a_camera_adjust, v3a_camera_adjust_backward,
v3a_gs_project_backward_cam - through the C ABI: every tensor carved out of a poisoned arena (offset 16 moves the views off their
256-byte alignment and keeps the 16 bytes the entry gradients' vector loads need), the workspace at exactly its queried size.  No
byte outside the views changes, the inputs keep their bits, the results are bit-equal to the plain calls of ops, and a workspace
one word short is refused."""
import ctypes as C
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guard as G  # noqa: E402
import pose_opt_oracle as PO  # noqa: E402
import test_pose_opt_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

p = lambda t: C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _clean(parity, tag, outputs, **info):
    torch.cuda.synchronize()
    bad = {n: G.violations(t) for n, t in outputs.items()}
    print(f"[pose guard {tag}] {info}; violations { {n: v[0] for n, v in bad.items()} }")
    parity(f"pose_opt::guard_{tag}", violations=sum(v[0] for v in bad.values()), **info)
    for n, (cnt, where) in bad.items():
        assert cnt == 0, (n, cnt, where)


@pytest.mark.parametrize("V,offset", [(1, 0), (3, 16), (13, 16), (65, 0)])
def test_camera_adjust(hip_lib, parity, V, offset):
    from vist3a_amd import ops
    L = hip_lib
    c2w = PO.cameras(V, 5, torch.float32).cuda()
    w2c = torch.linalg.inv(c2w).contiguous()
    d = PO.deltas(V, 6, 0.3, torch.float32).cuda()
    g = torch.Generator().manual_seed(7)
    gv, gc = torch.randn(V, 4, 4, generator=g).cuda(), torch.randn(V, 3, generator=g).cuda()
    dd = d.clone().requires_grad_(True)
    view, campos = ops.camera_adjust(w2c, c2w, dd)
    gd, = torch.autograd.grad((view * gv).sum() + (campos * gc).sum(), dd)
    ins = {n: G.carve_like(t, offset_bytes=offset) for n, t in dict(w2c=w2c, c2w=c2w, d=d, gv=gv, gc=gc).items()}
    fill = lambda *s: G.carve_like(torch.full(s, 3.0, device="cuda"), offset_bytes=offset)
    o_view, o_campos, o_d = fill(V, 4, 4), fill(V, 3), fill(V, 9)
    assert L.v3a_camera_adjust(p(ins["w2c"]), p(ins["c2w"]), p(ins["d"]), V, p(o_view), p(o_campos), _stream()) == 0
    assert L.v3a_camera_adjust_backward(p(ins["w2c"]), p(ins["c2w"]), p(ins["d"]), p(ins["gv"]), p(ins["gc"]), V, p(o_d), _stream()) == 0
    _clean(parity, "camera_adjust", dict(viewmat=o_view, campos=o_campos, d_deltas=o_d), V=V, offset=offset)
    for n, t in dict(w2c=w2c, c2w=c2w, d=d, gv=gv, gc=gc).items():
        assert G.unchanged(ins[n], t), n
    assert torch.equal(G.bits(o_view), G.bits(view.detach())) and torch.equal(G.bits(o_campos), G.bits(campos.detach()))
    assert torch.equal(G.bits(o_d), G.bits(gd))


@pytest.mark.parametrize("U,Cn,deg,layout,aa,offset", [(1, 1, 0, 1, False, 16), (65, 3, 4, 1, True, 0), (1027, 3, 3, 0, False, 16),
                                                        (20001, 1, 4, 1, False, 0), (1027, 1, 4, 1, True, 16)])
def test_project_backward_cam(hip_lib, parity, U, Cn, deg, layout, aa, offset):
    from vist3a_amd import lib, ops
    L = hip_lib
    cs = T._project_case(ops, U, Cn, deg, layout, aa)
    tight = T._project_bwd(ops, cs, deg, layout, aa)
    means, cov, shl, view, campos, K = cs["dev"]
    sh_k = 25
    eg = [t.cuda() for t in cs["cot"]]
    opac = cs["op"].cuda()
    src = dict(means=means, cov=cov, sh=shl, view=view, campos=campos, K=K, radii=cs["radii"], vm2=eg[0], vcon=eg[1], vcol=eg[2],
               vop=eg[3], opac=opac)
    ins = {n: G.carve_like(t.contiguous(), offset_bytes=offset) for n, t in src.items()}
    fill = lambda like: G.carve_like(torch.full_like(like, 3.0), offset_bytes=offset)
    outs = dict(d_means=fill(means), d_covars=fill(cov), d_sh=fill(shl), d_opacities=fill(opac), d_viewmat=fill(view), d_campos=fill(campos))
    need = int(L.v3a_gs_project_backward_cam_workspace_bytes(U, Cn))
    assert need == 120 * ((U + 63) // 64) * Cn
    g_ws = G.carve((need // 8,), torch.float64, device="cuda")
    a = lib.GsProjectBackwardArgs(p(ins["means"]), p(ins["cov"]), p(ins["sh"]), layout, sh_k, deg, p(ins["view"]), p(ins["campos"]), p(ins["K"]),
                                  U, Cn, cs["W"], cs["H"], 0.3, p(ins["radii"]), p(ins["vm2"]), p(ins["vcon"]), p(ins["vcol"]), p(ins["vop"]),
                                  p(outs["d_means"]), p(outs["d_covars"]), p(outs["d_sh"]), p(outs["d_opacities"]), int(aa),
                                  p(ins["opac"]) if aa else None)
    call = lambda nbytes: L.v3a_gs_project_backward_cam(C.byref(a), p(outs["d_viewmat"]), p(outs["d_campos"]), p(g_ws), nbytes, _stream())
    assert call(need - 8) == -4                                                      # held to its queried size
    assert call(need) == 0
    _clean(parity, "project_backward_cam", dict(workspace=g_ws, **outs), U=U, C=Cn, deg=deg, layout=layout, antialiased=aa, offset=offset,
           workspace_bytes=need)
    for n, t in src.items():
        assert G.unchanged(ins[n], t.contiguous()), n
    for o, t in zip(("d_means", "d_covars", "d_sh", "d_opacities", "d_viewmat", "d_campos"), tight):
        assert torch.equal(G.bits(outs[o]), G.bits(t)), o
