"""The cases of tests/recon_tail_cases.py judged by the oracles alone, no GPU needed.

  * Oracle agreement: the restatements reproduce oracle/recon.py (upsample_T, unproject, gaussian_adapter + map_pdf_to_opacity +
    sh_mask, quat_to_mat) and torch (F.interpolate, F.softplus, sigmoid, scaled_dot_product_attention, F.linear) in fp64 to 1e-12.
  * Census: every named branch group of every constructor has the stated size, counted from the inputs.
  * Mutants: a restatement with exactly ONE rule changed, run in fp32 as a kernel would run it (several rules differ from the true
    one only through fp32 overflow: softplus without its threshold is inf, then capped, from x = 89 on), is judged by the metric of
    tests/test_recon_tail_gpu.py against the true fp64 oracle on every case the rule concerns, and must miss that case's gate,
    min(4 x e32, 1e-3), by more than 10x on at least one output.  Where the gate is bit equality (e32 = 0) "10x" is taken from the
    output format's unit roundoff instead (2^-8 for the bf16 temporal upsample, 2^-24 otherwise).  So a kernel that got the rule
    wrong would fail the GPU test, and that is shown without touching a kernel.
  * Finiteness and exactness: e32 is finite for every case, and zero exactly where the case was built to be exact."""
import math

import pytest
import torch
import torch.nn.functional as F

import recon_tail_cases as T
from oracle import recon as R

F64, F32 = torch.float64, torch.float32
KERNEL_CASES = dict(adapter=lambda: [T.adapter_case(d, 67, pad, e) for d in range(5) for pad in T.ADAPTER_PAD for e in T.ADAPTER_EXP],
                    unproject=T.unproject_cases, bilinear=T.all_bilinear_cases, upsample_t=T.upsample_t_cases, linear=T.linear_cases,
                    attention=T.attention_cases)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.fixture
def default_f64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    yield
    torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------ oracle agreement
def test_softplus_sigmoid_and_quat_to_mat_agree_with_torch_and_the_oracle():
    x = torch.tensor(T.SOFTPLUS_X + (19.999, 20.001, -5.0, 3.0), dtype=F64)
    assert _rel(T.softplus(x), F.softplus(x)) <= 1e-12
    d = torch.tensor(T.DENSITY_X, dtype=F64)
    assert _rel(1 / (1 + torch.exp(-d)), torch.sigmoid(d)) <= 1e-12
    q = torch.randn(50, 4, dtype=F64, generator=torch.Generator().manual_seed(1)) * torch.logspace(-6, 6, 50, dtype=F64)[:, None]
    assert _rel(T.quat_to_mat(q), R.quat_to_mat(q)) <= 1e-12


@pytest.mark.parametrize("deg", range(5))
@pytest.mark.parametrize("op_exp", T.ADAPTER_EXP)
def test_adapter_oracle_agrees_with_the_reconstruction_oracle(deg, op_exp):
    case = T.adapter_case(deg, 67, 5, op_exp)
    mine = T.adapter_oracle(case, F64)
    dsh = (deg + 1) ** 2
    f = case["feats"][:, :8 + 3 * dsh].double()
    opac = R.map_pdf_to_opacity(torch.sigmoid(f[:, 0]), initial=math.log2(op_exp), final=math.log2(op_exp))
    ref = R.gaussian_adapter(case["pts"].double(), opac, f[:, 1:], sh_degree=deg)
    for n in T.ADAPTER_OUTPUTS:
        assert mine[n].shape == ref[n].shape, n
        assert T.per_row_error(mine[n].reshape(67, -1), ref[n].double().reshape(67, -1)) <= 1e-12, n


def test_unproject_oracle_agrees_with_the_reconstruction_oracle(default_f64):
    S, H, W = 3, 5, 7
    case = T.unproject_case(S, H, W, 8)
    f = torch.arange(S, dtype=F64)
    q = torch.stack([0.5 + 0.1 * f, -0.3 - 0.05 * f, 0.7 - 0.15 * f, 0.4 + 0.02 * f], -1)
    Rm = R.quat_to_mat(q)                                  # orthonormal to fp64 rounding, so (R^T, -R^T t) <-> (R, t) loses nothing
    t = case["t"]
    k = case["cam"][:, :4].double()
    Rt = Rm.transpose(1, 2)
    cam = torch.cat([k, Rt.reshape(S, 9), -(Rt @ t[:, :, None])[:, :, 0]], 1)
    mine = T.unproject_oracle(dict(case, cam=cam), F64)
    K = torch.zeros(1, S, 3, 3)
    K[0, :, 0, 0], K[0, :, 1, 1], K[0, :, 0, 2], K[0, :, 1, 2], K[0, :, 2, 2] = k[:, 0], k[:, 1], k[:, 2], k[:, 3], 1.0
    ext = torch.cat([Rm, t[:, :, None]], -1)[None]
    raw = case["raw"].double()
    ref = R.unproject(raw[:, 0].exp().view(1, S, H, W), ext, K)[0]
    assert T.per_row_error(mine["pts"], ref.reshape(-1, 3)) <= 1e-12
    assert _rel(mine["conf"][:, 0], 1 + raw[:, 1].exp()) <= 1e-12 and _rel(mine["depth"][:, 0], raw[:, 0].exp()) <= 1e-12


@pytest.mark.parametrize("hw,HW", T.BILINEAR_SHAPES)
@pytest.mark.parametrize("align", [False, True])
def test_bilinear_oracle_agrees_with_interpolate(hw, HW, align):
    for case in T.bilinear_cases(hw, HW, align):
        ref = F.interpolate(case["x"].double().permute(0, 3, 1, 2), size=HW, mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
        if case["add"] is not None:
            ref = ref + case["add"].double()
        if case["table"] is not None:
            ref = ref + case["table"].double().view(1, *HW, -1)
        if case["relu"]:
            ref = ref.relu()
        assert _rel(T.bilinear_oracle(case, F64), ref) <= 1e-12, case["name"]


@pytest.mark.parametrize("Tl,C,hw", T.UPT_CASES)
def test_upsample_t_oracle_agrees_with_the_reconstruction_oracle(Tl, C, hw):
    case = T.upsample_t_case(Tl, C, hw)
    ref = R.upsample_T(case["z"].double()[None])[0].permute(1, 2, 3, 0)
    assert _rel(T.upsample_t_oracle(case, F64), ref) <= 1e-12


@pytest.mark.parametrize("spec", T.LINEAR_CASES, ids=lambda s: "-".join(map(str, s)))
def test_linear_oracle_agrees_with_torch(spec):
    c = T.linear_case(*spec)
    ref = {"none": lambda t: t, "gelu": F.gelu, "silu": F.silu, "relu": F.relu}[c["act"]](F.linear(c["x"].double(), c["w"].double(), c["b"].double()))
    if c["gamma"] is not None:
        ref = c["res"].double() + c["gamma"].double() * ref
    assert _rel(T.linear_oracle(c, F64), ref) <= 1e-12


@pytest.mark.parametrize("spec", T.ATTENTION_CASES, ids=lambda s: "-".join(map(str, s)))
def test_attention_oracle_agrees_with_sdpa(spec):
    c = T.attention_case(*spec)
    S, H, hd = spec[:3]
    q, k, v = c["qkv"].double().view(S, 3, H, hd).permute(1, 2, 0, 3)
    ref = F.scaled_dot_product_attention(q[None], k[None], v[None])[0].permute(1, 0, 2).reshape(S, H * hd)
    assert _rel(T.attention_oracle(c, F64), ref) <= 1e-12


# ------------------------------------------------------------------------------------------------ census
@pytest.mark.parametrize("deg", range(5))
@pytest.mark.parametrize("pad", T.ADAPTER_PAD)
def test_adapter_census(deg, pad):
    case = T.adapter_case(deg, 67, pad, 1.0)
    c = T.adapter_census(case)
    dsh = (deg + 1) ** 2
    assert case["feats"].shape == (67, 8 + 3 * dsh + pad) and 3 * dsh == (3, 12, 27, 48, 75)[deg]
    assert sum(c["softplus"].values()) == 201 and min(c["softplus"].values()) >= 20        # 201 scale logits over 10 values
    assert sum(c["density"].values()) == 67 and min(c["density"].values()) >= 13           # 67 rows over 5 logits
    assert sum(c["quat"].values()) == 67 and min(c["quat"].values()) >= 11, c["quat"]      # 67 rows over 6 groups
    assert c["quat"] == {n: int((case["groups"]["quat"] == i).sum()) for i, n in enumerate(T.QUAT_GROUPS)}
    # what each group is for, from the fp64 oracle's values: pass-through above 20, cap from 300 on, exp underflow at -110
    assert c["passthrough"] == sum(c["softplus"][v] for v in (20.5, 50.0, 299.0, 301.0, 1000.0))
    assert c["capped"] == c["softplus"][301.0] + c["softplus"][1000.0] and c["exp_underflows"] == c["softplus"][-110.0]
    o = T.adapter_oracle(case, F64)
    x = case["feats"][:, 1:4].double()
    assert bool((o["scales"][x >= 301] == 0.3).all()) and bool((o["scales"][x == 299.0] < 0.3).all())
    assert float(T.adapter_oracle(case, F32)["scales"][x == -110.0].abs().max()) == 0
    assert c["zero_quat"] == 0 and c["subnormal_exp_args"] == 0 and c["negative_w_rows"] >= c["quat"]["negw"] >= 4
    assert bool(torch.isnan(case["feats"][:, 8 + 3 * dsh:]).all()) and not bool(torch.isnan(case["feats"][:, :8 + 3 * dsh]).any())
    d = case["feats"][:, 0].double()                      # fp32: logits of +-100 and +20 saturate the sigmoid, -20 does not
    p32 = T.adapter_oracle(case, F32)["opacities"]
    assert bool((p32[d == -100] == 0).all()) and bool((p32[d >= 20] == 1).all()) and bool(((p32[d == -20] > 0) & (p32[d == -20] < 1e-8)).all())
    assert bool((p32[d == 0] == 0.5).all())


def test_adapter_launch_sizes_leave_partial_groups_and_waves():
    for U in T.ADAPTER_U:
        sizes = [min(U, 67 - r0) for r0 in range(0, 67, U)]
        assert sum(sizes) == 67
    assert {67 % U for U in T.ADAPTER_U} == {0, 1, 3, 2}        # ragged last launches of 1, 3 and 2 rows as well
    assert all(U % 4 for U in (1, 3, 5, 67))                    # a wave holds four Gaussians: these leave one partly idle


@pytest.mark.parametrize("S,H,W", T.UNPROJECT_SHAPES)
@pytest.mark.parametrize("ld", T.UNPROJECT_LD)
def test_unproject_census(S, H, W, ld):
    case = T.unproject_case(S, H, W, ld)
    c = T.unproject_census(case)
    assert c["per_frame"] == [H * W] * S and case["raw"].shape == (S * H * W, ld)
    assert c["fx_ne_fy"] and c["cx_ne_cy"] and c["cameras_distinct"] and c["t_components_differ"]
    assert c["min_asymmetry"] > 1.0                        # ||R - R^T||_F; 0 for a symmetric rotation, at most 2 sqrt 2
    assert -3 <= c["raw_min"] and c["raw_max"] <= 3
    assert c["straddling_blocks"] == {(1, 1, 1): 0, (3, 5, 7): 1, (2, 16, 17): 1, (4, 9, 30): 3}[(S, H, W)]
    if ld > 2:
        assert bool(torch.isnan(case["raw"][:, 2:]).all())
    cx, cy = case["cam"][:, 2].double(), case["cam"][:, 3].double()
    assert bool((cx != cx.round()).all()) and bool((cy != cy.round()).all())       # u - cx is never 0


@pytest.mark.parametrize("hw,HW", T.BILINEAR_SHAPES)
@pytest.mark.parametrize("align", [False, True])
def test_bilinear_census(hw, HW, align):
    cases = T.bilinear_cases(hw, HW, align)
    assert sorted((c["add"] is not None, c["table"] is not None, c["relu"]) for c in cases) == sorted(T.BILINEAR_FLAGS)
    assert {c["x"].shape[0] for c in cases} == {1, 3} and {c["x"].shape[3] for c in cases} == {8, 24}
    (h, w), (H, W) = hw, HW
    for case in cases:
        c = T.bilinear_census(case)
        Tn = case["x"].shape[0]
        # the same sets from the fp64 oracle's own coordinates
        sy, sx = T._src(H, h, align, F64), T._src(W, w, align, F64)
        ry, rx = T._src(H, h, align, F64, True), T._src(W, w, align, F64, True)
        assert [int(i) for i in (sy.floor() == h - 1).nonzero()] == c["last_y"] and [int(i) for i in (sx.floor() == w - 1).nonzero()] == c["last_x"]
        assert [int(i) for i in (ry < 0).nonzero()] == c["zero_y"] and [int(i) for i in (rx < 0).nonzero()] == c["zero_x"]
        for n in ("last", "clamped0"):                     # a group is empty by construction (stated below) or has >= 4 members
            assert c[n] == 0 or c[n] >= 4, (case["name"], n, c[n])
        per_frame = {((4, 6), (8, 12)): (8 + 12 - 1, 19), ((5, 5), (5, 5)): (9, 9), ((3, 4), (7, 9)): (7 + 9 - 1, 15),
                     ((7, 9), (3, 4)): (0, 6), ((1, 5), (4, 5)): (20, 20), ((5, 1), (5, 3)): (15, 15), ((6, 6), (1, 1)): (0, 0)}[(hw, HW)]
        assert c["last"] == Tn * per_frame[int(align)], (case["name"], c["last"])
        zero = {((4, 6), (8, 12)): 19, ((3, 4), (7, 9)): 7 + 9 - 1, ((1, 5), (4, 5)): 5 * 2, ((5, 1), (5, 3)): 5}.get((hw, HW), 0)
        assert c["clamped0"] == (0 if align else Tn * zero), (case["name"], c["clamped0"])


@pytest.mark.parametrize("Tl,C,hw", T.UPT_CASES)
def test_upsample_t_census(Tl, C, hw):
    case = T.upsample_t_case(Tl, C, hw)
    c = T.upsample_t_census(case)
    assert c["frames"] == 4 * (Tl - 1) + 1 and len(c["copied"]) == Tl and len(c["blended"]) == 3 * (Tl - 1)
    z = case["z"]
    assert float(z.abs().max()) <= 4 and bool((z * 64 == (z * 64).round()).all())
    o = T.upsample_t_oracle(case, F64)
    for i, t in enumerate(c["copied"]):                    # frames with t % 4 == 0 are the latent frames themselves
        assert torch.equal(o[t], z[:, i].double().permute(1, 2, 0))
    assert torch.equal(T.upsample_t_oracle(case, F32).double(), o)     # l0 a + l1 b is exact in fp32: only the bf16 rounding is left


def test_linear_census():
    specs = T.LINEAR_CASES
    cs = {s: T.linear_census(T.linear_case(*s)) for s in specs}
    Ms, Ns, Ks = ({s[i] for s in specs} for i in range(3))
    assert Ms == {1, 16, 17, 32} and Ns >= {1, 5, 9, 33} and Ks == {4, 12, 256, 260, 508}
    assert (17, 260) in {(s[0], s[2]) for s in specs} and (32, 33) in {(s[0], s[1]) for s in specs}
    assert {s[3] for s in specs} == {"none", "gelu", "silu", "relu"} and {s[4] for s in specs} == {False, True}
    # the host's choice, replayed: up to N = 1024 one output per wave gives the most workgroups (N = 1: all counts tie, the largest wins)
    assert all(T.linear_npw(M, N) == (4 if (N == 1 and M <= 16) else 2 if N == 1 else 1) for M in (1, 16, 17, 32) for N in (1, 5, 9, 33, 1024))
    assert {c["instantiation"] for c in cs.values()} == {(16, 1), (16, 2), (16, 3), (16, 4), (32, 1), (32, 2)}
    assert cs[(32, 1029, 12, "none", False, "randn")] | dict(chunks=0, last_chunk_floats=0, rereading_lanes=0) == dict(
        instantiation=(32, 2), workgroups=129, idle_waves=1, partly_valid_waves=1, dropped_in_partly_valid=1, chunks=0, last_chunk_floats=0,
        rereading_lanes=0)
    c = cs[(16, 1027, 260, "none", False, "tail")]
    assert (c["instantiation"], c["partly_valid_waves"], c["dropped_in_partly_valid"], c["idle_waves"], c["last_chunk_floats"]) == ((16, 2), 1, 1, 2, 4)
    c = cs[(16, 2999, 12, "silu", True, "randn")]
    assert (c["instantiation"], c["partly_valid_waves"], c["dropped_in_partly_valid"], c["idle_waves"]) == ((16, 3), 1, 1, 0)
    c = cs[(1, 1, 4, "none", False, "dyadic")]
    assert (c["instantiation"], c["partly_valid_waves"], c["dropped_in_partly_valid"], c["idle_waves"]) == ((16, 4), 1, 3, 3)
    # with one output per wave a wave is live or idle, never partly valid; idle waves occur whenever N is no multiple of 4
    for s, c in cs.items():
        if c["instantiation"][1] == 1:
            assert c["partly_valid_waves"] == 0 and c["idle_waves"] == -s[1] % 4, s
    assert {c["idle_waves"] for c in cs.values()} >= {1, 2, 3}
    assert {c["chunks"] for c in cs.values()} == {1, 2} and {c["last_chunk_floats"] for c in cs.values()} == {4, 12, 256, 252}
    assert {c["rereading_lanes"] for c in cs.values()} >= {63, 1, 0}            # K = 260 / 4: one live lane; K = 508: one re-reading lane
    tails = [T.linear_case(*s) for s in specs if s[5] == "tail"]
    assert len(tails) >= 2 and {t["x"].shape[1] for t in tails} == {260, 508}
    for t in tails:
        assert bool((t["x"][:, -4:] == 1e6).all()) and bool((t["w"][:, -4:] == 1e6).all()) and float(t["x"][:, :-4].abs().max()) < 10


def test_attention_census():
    assert {s[:3] for s in T.ATTENTION_CASES} == {(1, 1, 128), (2, 3, 8), (13, 2, 32), (64, 1, 64), (33, 4, 128)}
    for s in T.ATTENTION_CASES:
        c = T.attention_census(T.attention_case(*s))
        assert c["rows"] == s[0] * s[1]
        assert (3 * s[0] * s[2] + 64) * 4 <= 64 * 1024                  # the kernel's LDS limit
        if s[3] > 1:     # +-40: one key holds the softmax of every row
            assert c["max_score"] == pytest.approx(40, abs=1e-4) and c["min_score"] == pytest.approx(-40, abs=1e-4)
            assert c["dominated_rows"] == c["rows"] >= 4
        else:
            assert abs(c["max_score"]) < 8 and c["dominated_rows"] == (c["rows"] if s[0] == 1 else 0)
    assert {max(0, 64 - s[2]) for s in T.ATTENTION_CASES} == {0, 56, 32}      # hd 8 and 32 leave PV lanes idle


def test_saturation_cases_hold_what_they_say():
    for e in T.ADAPTER_EXP:
        c = T.adapter_saturation_case(e)
        q, d = c["feats"][:, 4:8], c["feats"][:, 0]
        assert int((q.abs().sum(-1) == 0).sum()) == 4 and int((q.norm(dim=-1) > 1e24).sum()) == 4
        assert int((d == 100).sum()) == 4 and int((d == -100).sum()) == 4
        o = T.adapter_oracle(c, F32)
        assert bool(torch.isnan(o["covariances"][:8]).all()) and bool(torch.isfinite(o["covariances"][8:]).all())
        assert bool(torch.isfinite(o["rotations"]).all()) and bool(torch.isfinite(o["scales"]).all())
        o64 = T.adapter_oracle(c, F64)
        ordinary, sat = T.saturation_split(o["rotations"], o64["rotations"])          # 1e25 q / inf = 0 in fp32, a unit quaternion in fp64
        assert sat.tolist() == [False] * 4 + [True] * 4 + [False] * 8 and ordinary.tolist() == [True] * 4 + [False] * 4 + [True] * 8
        ordinary, sat = T.saturation_split(o["covariances"].reshape(16, -1), o64["covariances"].reshape(16, -1))
        assert not bool(sat.any()) and ordinary.tolist() == [False] * 8 + [True] * 8
    c = T.unproject_saturation_case()
    r = c["raw"]
    for col in (0, 1):
        assert int((r[:, col] == 100).sum()) >= 4 and int((r[:, col] == -110).sum()) >= 4
    o = T.unproject_oracle(c, F32)
    cls = T.value_class(o["pts"])
    assert int((cls != 0).sum()) > 0 and bool(torch.isposinf(o["depth"][r[:, 0] == 100]).all()) and bool((o["depth"][r[:, 0] == -110] == 0).all())
    assert bool(torch.isposinf(o["conf"][r[:, 1] == 100]).all()) and bool((o["conf"][r[:, 1] == -110] == 1).all())
    for n in T.UNPROJECT_OUTPUTS:                          # exp(-110) = 0 and 1 + 0 are within the metric's floor of fp64: ordinary rows
        ordinary, sat = T.saturation_split(o[n], T.unproject_oracle(c, F64)[n])
        assert not bool(sat.any()) and bool((ordinary == torch.isfinite(o[n]).all(1)).all()), n


# ------------------------------------------------------------------------------------------------ e32 and the mutants
@pytest.mark.parametrize("kernel", list(KERNEL_CASES))
def test_fp32_oracle_error_is_finite_and_zero_where_the_case_is_exact(kernel):
    for case in KERNEL_CASES[kernel]():
        _, e32, gate = T.reference(kernel, case)
        for n, e in e32.items():
            assert math.isfinite(e) and 0 <= e < T.CEILING / 4, (case["name"], n, e)
            exact = {"adapter": n == "means" or (n == "harmonics" and case.get("sh_degree") == 0), "upsample_t": True,
                     "linear": case.get("kind") == "dyadic", "attention": kernel == "attention" and case["qkv"].shape[0] == 1,
                     "bilinear": kernel == "bilinear" and case["exact"] and (not case["align"] or case["size"] == (5, 5)),
                     "unproject": False}[kernel]
            # (bilinear: resizes along an axis of one source row / column, and to 1 x 1, have dyadic or no weights and are exact too)
            assert e == 0 if exact else (e > 0 or kernel == "bilinear"), (case["name"], n, e)


@pytest.mark.parametrize("kernel,mutant", [(k, m) for k, ms in T.MUTANTS.items() for m in ms])
def test_mutant_misses_the_gate_tenfold(kernel, mutant):
    applies = T.MUTANTS[kernel][mutant]
    cases = [c for c in KERNEL_CASES[kernel]() if applies(c)]
    assert len(cases) >= 3, (kernel, mutant, len(cases))
    unit = 2.0 ** -8 if kernel == "upsample_t" else 2.0 ** -24
    weakest = math.inf
    for case in cases:
        r64, e32, gate = T.reference(kernel, case)
        got = T.as_rows(kernel, T.ORACLES[kernel](case, F32, mutant))
        ratio = max(T.per_row_error(got[n], r64[n]) / max(gate[n], unit) for n in r64)
        weakest = min(weakest, ratio)
        assert ratio > 10, (case["name"], mutant, ratio)
    print(f"{kernel}/{mutant}: {len(cases)} cases, weakest miss {weakest:.3g} x the gate")


def test_each_kernel_has_three_mutants():
    assert set(T.MUTANTS) == set(T.ORACLES) and all(len(m) >= 3 for m in T.MUTANTS.values())
