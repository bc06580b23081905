"""Host-side checks of pose optimisation (csrc/post_opt.hip v3a_camera_adjust*, csrc/raster_bwd.hip v3a_gs_project_backward_cam,
vist3a_amd.post_opt), no GPU needed.

  * tests/pose_opt_oracle.py against tensors recorded from the reference's CameraOptModule (1e-13: the two are the same fp64
    operations; a product order is all that may differ);
  * the closed form the kernel uses, [Rd^T | -Rd^T dx] w2c, against torch.linalg.inv(c2w T) in fp64;
  * the YARDSTICK of the GPU tests' camera gradients: torch.autograd through oracle/gsplat_raster.py with respect to viewmat and
    campos in fp64 agrees with central finite differences.  As in tests/test_raster_bwd_host.py: h = 1e-6 along random directions;
    a camera entry is of order 1 (rotation) to 4 (depth of the scene), so the relative step is >= 2.5e-7 and the truncation term
    ~h^2 = 1e-12 times a modest derivative ratio; rounding is |loss| x 2^-53 / h ~ 1e3 x 1e-16 / 1e-6 = 1e-7 against directional
    derivatives of order 10 .. 1000 (a camera moves EVERY Gaussian, so they are larger than a Gaussian's own).  Bound: 1e-6
    relative, the same as there;
  * argument validation and the workspace query of the three new entry points (null stream, nothing launched);
  * PostOptConfig.check_pose, the CLI flags, and the pose Adam (rate schedule + weight decay) against torch.optim.Adam(weight_decay)
    + ExponentialLR on the CPU."""
import ctypes
import math
import sys
from pathlib import Path

import pytest
import torch
from safetensors.torch import load_file

from oracle import gsplat_raster as G

sys.path.insert(0, str(Path(__file__).resolve().parent))
import pose_opt_oracle as PO  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden" / "pose_opt_ref.safetensors"


@pytest.mark.parametrize("case", sorted(PO.GOLDEN_CASES))
def test_oracle_matches_reference_module(case):
    gold = load_file(str(GOLD))
    c2w, d = gold[case + ".c2w"], gold[case + ".deltas"]
    assert c2w.dtype == torch.float64 and tuple(d.shape) == (3, 9)
    out = PO.adjust(c2w, d)
    view, campos = PO.camera_adjust(c2w, d)
    e = [float((a - gold[case + k]).abs().max()) for a, k in ((out, ".out"), (view, ".viewmat"), (campos, ".campos"))]
    print(f"[pose oracle {case}] max abs difference to the reference's module: c2w' {e[0]:.2e}  viewmat {e[1]:.2e}  campos {e[2]:.2e}")
    assert max(e) <= 1e-13
    if case == "zero":
        assert torch.equal(out, c2w)


@pytest.mark.parametrize("size", [0.0, 1e-2, 0.5])
def test_closed_form_is_the_inverse(size):
    c2w, d = PO.cameras(5, 7), PO.deltas(5, 8, size)
    w2c = torch.linalg.inv(c2w)
    v_ref, p_ref = PO.camera_adjust(c2w, d)
    v, p = PO.closed_form(w2c, c2w, d)
    ev, ep = float((v - v_ref).abs().max()), float((p - p_ref).abs().max())
    print(f"[closed form |delta| {size}] viewmat {ev:.2e}  campos {ep:.2e}")
    # entries of order 1 .. 5, two 4x4 products and an LU inverse apart: a few hundred eps_fp64
    assert ev <= 1e-13 and ep <= 1e-13
    T = PO.transform(d)
    R = T[:, :3, :3]
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14      # a rotation
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-14


def _scene(U, seed, K=9):
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(U, 3, generator=g) * torch.tensor([1.2, 1.2, 1.0]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(U, 3, 3, generator=g) * 0.2
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)
    sh = torch.randn(U, K, 3, generator=g) * 0.3
    return means.double(), cov.double(), sh.double()


def test_oracle_camera_gradient_matches_finite_differences(monkeypatch):
    U, W, H, deg = 60, 48, 40, 2
    means, cov, sh = _scene(U, 5)
    c, s = math.cos(0.15), math.sin(0.15)
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float64)
    view[:3, 3] = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
    campos = torch.linalg.inv(view)[:3, 3].clone()
    K = torch.tensor([[50.0, 0, W / 2], [0, 55.0, H / 2], [0, 0, 1.0]], dtype=torch.float64)
    g = torch.Generator().manual_seed(6)
    wm, wc, wcol = (torch.randn(U, n, generator=g, dtype=torch.float64) for n in (2, 3, 4))

    def loss(v, cp):
        with monkeypatch.context() as m:
            m.setattr(G, "f32", torch.float64)
            p = G.project(means, cov, v, K, W, H)
            col = G.sh_colors(means, cp, sh, deg)
        col4 = torch.cat([col, p["depths"][:, None]], -1)
        return (p["means2d"] * wm).sum() + (p["conics"] * wc).sum() + (col4 * wcol).sum()

    v, cp = view.clone().requires_grad_(True), campos.clone().requires_grad_(True)
    gv, gc = torch.autograd.grad(loss(v, cp), (v, cp))
    assert float(gv[3].abs().max()) == 0                       # the bottom row is not read
    h = 1e-6
    for k in range(4):
        dv = torch.zeros(4, 4, dtype=torch.float64)
        dv[:3] = torch.randn(3, 4, generator=g, dtype=torch.float64)
        dc = torch.randn(3, generator=g, dtype=torch.float64)
        for a, b, name in ((dv, torch.zeros(3, dtype=torch.float64), "viewmat"), (torch.zeros(4, 4, dtype=torch.float64), dc, "campos")):
            with torch.no_grad():
                fd = float(loss(view + h * a, campos + h * b) - loss(view - h * a, campos - h * b)) / (2 * h)
            an = float((gv * a).sum() + (gc * b).sum())
            err = abs(fd - an) / max(abs(an), 1.0)
            print(f"[fd {name} dir {k}] autograd {an:+.6e}  finite difference {fd:+.6e}  error {err:.2e}")
            assert err <= 1e-6, (name, k, an, fd)


def test_new_entry_points_validate_without_gpu():
    from vist3a_amd import lib
    L = lib.load()
    assert L.v3a_abi_version() == lib.EXPECTED_ABI >= 32
    # workspace query: one row of 15 doubles per wave of 64 Gaussians and camera
    q = L.v3a_gs_project_backward_cam_workspace_bytes
    assert q(1, 1) == 120 and q(64, 1) == 120 and q(65, 1) == 240 and q(20001, 3) == 3 * 313 * 120 and q(0, 2) == 0
    assert q(2_400_000, 1) == 37500 * 120
    assert q(-1, 1) == -2 and q(10, 0) == -2 and q(1 << 31, 1) == -2
    f = L.v3a_gs_project_backward_cam
    assert f(None, 8, 8, 8, 1 << 20, None) == -1
    p = lib.GsProjectBackwardArgs()
    assert f(ctypes.byref(p), 8, 8, 8, 1 << 20, None) == -1                   # null pointers in the struct
    for n in ("means", "covars", "sh", "viewmat", "campos", "K", "radii", "d_means2d", "d_conics", "d_colors", "d_opacity_partial",
              "d_means", "d_covars", "d_sh", "d_opacities"):
        setattr(p, n, 8)
    p.U, p.C, p.width, p.height, p.sh_k, p.sh_degree, p.sh_layout = 100, 2, 16, 16, 25, 4, 1
    for bad in ((None, 8, 8), (8, None, 8), (8, 8, None)):
        assert f(ctypes.byref(p), *bad, 1 << 20, None) == -1                   # d_viewmat, d_campos, workspace
    assert f(ctypes.byref(p), 8, 8, 12, 1 << 20, None) == -1                   # workspace not 8-byte aligned
    assert f(ctypes.byref(p), 8, 8, 8, 2 * 2 * 120 - 1, None) == -4            # one byte short
    p.sh_degree = 5
    assert f(ctypes.byref(p), 8, 8, 8, 1 << 20, None) == -2
    p.sh_degree, p.rasterize_mode = 4, 1
    assert f(ctypes.byref(p), 8, 8, 8, 1 << 20, None) == -1                   # antialiased without opacities
    p.rasterize_mode = 2
    assert f(ctypes.byref(p), 8, 8, 8, 1 << 20, None) == -1
    # camera_adjust, forward and backward
    fw, bw = L.v3a_camera_adjust, L.v3a_camera_adjust_backward
    for i in range(5):
        a = [8] * 5
        a[i] = None
        assert fw(a[0], a[1], a[2], 3, a[3], a[4], None) == -1
    for i in range(6):
        a = [8] * 6
        a[i] = None
        assert bw(a[0], a[1], a[2], a[3], a[4], 3, a[5], None) == -1
    for V in (0, -1, (1 << 24) + 1):
        assert fw(8, 8, 8, V, 8, 8, None) == -2 and bw(8, 8, 8, 8, 8, V, 8, None) == -2


def test_check_pose_and_schedule():
    from vist3a_amd.post_opt import PostOptConfig, pose_learning_rate
    cfg = PostOptConfig()
    assert cfg.pose_opt is False and cfg.pose_opt_lr == 1e-5 and cfg.pose_opt_reg == 1e-6
    cfg.check_pose()
    PostOptConfig(pose_opt=True).check_pose()
    PostOptConfig(pose_opt=False, pose_opt_lr=-1.0).check_pose()                # not looked at while off
    for bad in (dict(pose_opt_lr=0.0), dict(pose_opt_lr=-1e-5), dict(pose_opt_lr=float("nan")), dict(pose_opt_reg=-1e-6),
                dict(pose_opt_reg=float("nan")), dict(max_steps=0)):
        with pytest.raises(ValueError, match="PostOptConfig"):
            PostOptConfig(pose_opt=True, **bad).check_pose()
    with pytest.raises(ValueError, match="pose_opt must be a bool"):
        PostOptConfig(pose_opt=1).check_pose()
    cfg = PostOptConfig(pose_opt=True, max_steps=50, pose_opt_lr=2e-3)
    assert pose_learning_rate(cfg, 0) == 2e-3 and abs(pose_learning_rate(cfg, 50) / 2e-5 - 1) < 1e-12


def test_cli_flags_parse():
    from vist3a_amd.utils.argument import inference_vist3a_argument
    p = inference_vist3a_argument()
    req = ["--checkpoint_path", "c", "--transformer_lora_path", "l", "--input_texts_path", "t"]
    base = p.parse_args(req)
    assert base.post_opt_pose_opt is False and base.post_opt_pose_lr is None
    a = p.parse_args(req + ["--post_opt_steps", "5", "--post_opt_pose_opt", "--post_opt_pose_lr", "1e-4"])
    assert a.post_opt_pose_opt is True and a.post_opt_pose_lr == 1e-4 and a.post_opt_steps == 5


def _pose_transforms_match_oracle():
    from vist3a_amd.post_opt import pose_transforms
    d = PO.deltas(4, 3, 0.5)
    return float((pose_transforms(d.float()) - PO.transform(d.float().double())).abs().max())


def test_adjusted_extrinsics_host():
    from vist3a_amd.post_opt import PostOptConfig, adjusted_extrinsics
    assert _pose_transforms_match_oracle() <= 1e-15
    ext = PO.cameras(4, 11, torch.float32)
    cfg = PostOptConfig(pose_opt=True, test_every=2)           # views 1 and 3 train
    d = PO.deltas(2, 12, 0.1, torch.float32)
    out = adjusted_extrinsics(ext, dict(pose_deltas=d), cfg)
    assert torch.equal(out[0], ext[0]) and torch.equal(out[2], ext[2])          # held-out views as given
    want = PO.adjust(ext[[1, 3]].double(), d.double()).float()
    assert torch.equal(out[[1, 3]], want)
    assert torch.equal(adjusted_extrinsics(ext, {}, cfg), ext)
    assert torch.equal(adjusted_extrinsics(ext, dict(pose_deltas=torch.zeros(2, 9)), cfg), ext)
    with pytest.raises(ValueError, match="pose_deltas"):
        adjusted_extrinsics(ext, dict(pose_deltas=torch.zeros(4, 9)), cfg)


def _adam_restated(p, g, m, v, lr, t, eps=1e-8, b1=0.9, b2=0.999):
    """ops.adam_step's arithmetic (csrc/post_opt.hip adam_one) in fp64 on the host: what the loop's pose update computes"""
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    p.sub_(lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps))


def test_pose_adam_restatement_matches_torch():
    """The loop's update - adam_step(deltas, g + reg deltas, lr = pose_opt_lr 0.01^(s / max_steps), eps 1e-8) - against
    torch.optim.Adam(weight_decay=reg) + ExponentialLR(0.01^(1 / max_steps)) over 50 steps, both in fp64 on the CPU.  Recorded
    agreement: 1.975e-14 relative (largest over the elements and steps; an element that passes near zero sets it) - the two differ
    in how the rate's power is formed (one pow against a running product) and in the association of the bias corrections.
    Gate: 2x that, 4e-14."""
    from vist3a_amd.post_opt import PostOptConfig, pose_learning_rate
    cfg = PostOptConfig(pose_opt=True, max_steps=50, pose_opt_lr=1e-3, pose_opt_reg=1e-2)
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(3, 9, generator=g, dtype=torch.float64) * (1.0 if i % 7 else 0.0) for i in range(50)]
    ref = torch.zeros(3, 9, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([ref], lr=cfg.pose_opt_lr, weight_decay=cfg.pose_opt_reg)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.01 ** (1.0 / cfg.max_steps))
    p, m, v = (torch.zeros(3, 9, dtype=torch.float64) for _ in range(3))
    worst = 0.0
    for i, gr in enumerate(grads):
        ref.grad = gr.clone()
        opt.step()
        sched.step()
        _adam_restated(p, gr + cfg.pose_opt_reg * p, m, v, pose_learning_rate(cfg, i), i + 1)
        worst = max(worst, float(((p - ref.detach()).abs() / ref.detach().abs().clamp_min(1e-300)).max()))
    print(f"[pose adam] largest relative difference to torch.optim.Adam(weight_decay) + ExponentialLR over 50 steps: {worst:.3e}")
    assert float(ref.detach().abs().max()) > 1e-3
    assert worst <= 4e-14
