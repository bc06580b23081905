"""Branch-targeted inputs for the six small kernels of the reconstruction tail (csrc/elementwise.hip: gaussian_adapter,
depth_unproject, bilinear_cl, latent_upsample_t_cl, linear_f32, attention_small_f32), plain torch restatements of the six operations
that run in fp64 (the judge) and in fp32 (whose own error sets each gate), a census that proves from the inputs which elements take
which branch, and the per-row metric.  Plain module, CPU only; used by tests/test_recon_tail_host.py (oracle agreement, census,
mutants) and tests/test_recon_tail_gpu.py (HIP against fp64).

Every oracle takes exactly what the kernel takes (fp32 / bf16 tensors) and a dtype `dt` to compute in.  `mut` names ONE rule to
break; the host test shows that each broken rule misses the gates of the cases it concerns by more than 10x.

Metric: max over rows of ||got - ref64|| / (||ref64|| + floor), floor = 1e-3 x the median non-zero row norm; a row is a Gaussian,
a pixel or an output row; nothing is left out.  Gate: min(4 x e32, 1e-3), e32 = the fp32 oracle's own figure on the same metric
(device transcendentals and another summation order); e32 == 0 means the case is exact in fp32 and the gate is bit equality."""
import functools
import math

import torch

from oracle import recon as R

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
CEILING = 1e-3          # the project's per-kernel parity ceiling
NAN = float("nan")      # fills padding columns: whoever reads one poisons its output


# ------------------------------------------------------------------------------------------------ metric and gates
def per_row_error(got, ref64, keep=None):
    """max over rows r of ||got_r - ref_r|| / (||ref_r|| + floor).  Both [rows, ...].  `keep` (bool [rows]) restricts the rows
    (saturation cases only: the rows whose reference is finite); a non-finite figure comes back as inf."""
    n = ref64.shape[0]
    r = ref64.double().reshape(n, -1)
    g = got.detach().cpu().double().reshape(n, -1)
    if keep is not None:
        r, g = r[keep], g[keep]
        if r.shape[0] == 0:
            return 0.0
    nr = r.norm(dim=1)
    nz = nr[nr > 0]
    floor = 1e-3 * float(nz.median()) if nz.numel() else 1.0
    e = float(((g - r).norm(dim=1) / (nr + floor)).max())
    return e if math.isfinite(e) else math.inf


def saturation_split(ref32, ref64):
    """Rows of a saturation case, by what the fp32 run of the oracle makes of them -> (ordinary, saturated but finite), bool [rows].
    ordinary: finite in fp32 and within the ceiling of fp64 on the row metric; judged against fp64 like any other row.
    saturated but finite: finite in fp32 yet far from fp64 (1e25 q / inf = 0, exp(-110) = 0): every operation that made them had
    an exact 0 or inf operand, nothing was rounded, so the kernel must return the fp32 oracle's very values."""
    n = ref32.shape[0]
    r32, r64 = ref32.double().reshape(n, -1), ref64.double().reshape(n, -1)
    fin32 = torch.isfinite(r32).all(1)
    fin = fin32 & torch.isfinite(r64).all(1)
    nr = r64[fin].norm(dim=1)
    nz = nr[nr > 0]
    floor = 1e-3 * float(nz.median()) if nz.numel() else 1.0
    ordinary = fin.clone()
    ordinary[fin] = (r32[fin] - r64[fin]).norm(dim=1) / (nr + floor) <= CEILING
    return ordinary, fin32 & ~ordinary


def gate_from(e32):
    """4 x the fp32 oracle's own error on the same metric, never above the project's ceiling; 0 = bit equality"""
    return min(4.0 * e32, CEILING)


def passes(err, gate):
    return err == 0.0 if gate == 0.0 else err <= gate


def value_class(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element"""
    t = t.detach().cpu()
    return torch.isposinf(t).long() + 2 * torch.isneginf(t).long() + 3 * torch.isnan(t).long()


def grid(shape, g, step, lim=4.0):
    """random multiples of `step` in [-lim, lim]"""
    n = int(round(lim / step))
    return (torch.randint(-n, n + 1, shape, generator=g).double() * step).float()


def _balanced(n, k, g):
    """n group indices in 0 .. k-1, as evenly as n allows, in a seeded random order"""
    return (torch.arange(n) % k)[torch.randperm(n, generator=g)]


# ------------------------------------------------------------------------------------------------ gaussian adapter
SOFTPLUS_X = (-110.0, -30.0, 0.0, 19.5, 20.0, 20.5, 50.0, 299.0, 301.0, 1000.0)   # threshold 20, cap at 300, underflow below -104
DENSITY_X = (-100.0, -20.0, 0.0, 20.0, 100.0)
QUAT_GROUPS = ("unit", "small", "large", "tiny", "single", "negw")               # x 1e-3, x 1e3, x 1e-12, one component, w < 0
QUAT_SCALE = dict(unit=1.0, small=1e-3, large=1e3, tiny=1e-12, single=1.0, negw=1.0)
ADAPTER_ROWS = 67
ADAPTER_U = (1, 3, 4, 5, 67)
ADAPTER_PAD = (0, 5)
ADAPTER_EXP = (1.0, 2.0, 0.5)


def softplus(x):
    """F.softplus, beta 1, threshold 20"""
    return torch.where(x > 20, x, torch.log1p(torch.exp(x)))


def quat_to_mat(q):
    """xyzw quaternion -> rotation, the reference's formula (no normalisation assumed)"""
    i, j, k, r = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def opacity_map(pdf, e):
    return 0.5 * (1 - (1 - pdf) ** e + pdf ** (1 / e))


def adapter_oracle(case, dt, mut=None):
    """feats[u] = {density logit, 3 scale logits, 4 quaternion xyzw, 3 x dsh harmonics}; -> the kernel's six outputs, [U, ...].
    mut: no_threshold (softplus without its pass-through), no_cap, exp_one (the exponent-1 opacity path whatever the exponent),
    wxyz (quaternion read as wxyz)."""
    deg = case["sh_degree"]
    dsh = (deg + 1) ** 2
    f = case["feats"][:, :8 + 3 * dsh].to(dt)
    pdf = 1 / (1 + torch.exp(-f[:, 0]))
    opac = opacity_map(pdf, 1.0 if mut == "exp_one" else case["op_exp"])
    x = f[:, 1:4]
    sp = torch.log1p(torch.exp(x)) if mut == "no_threshold" else softplus(x)
    sc = 0.001 * sp
    if mut != "no_cap":
        sc = sc.clamp_max(0.3)
    q = f[:, 4:8]
    rot = q / ((q * q).sum(-1, keepdim=True).sqrt() + 1e-8)
    Rm = quat_to_mat(rot.roll(-1, -1) if mut == "wxyz" else rot)
    Sm = sc.diag_embed()
    cov = Rm @ Sm @ Sm.transpose(-1, -2) @ Rm.transpose(-1, -2)
    sh = f[:, 8:].reshape(-1, 3, dsh) * R.sh_mask(deg).to(dt)
    return dict(means=case["pts"].to(dt), covariances=cov, harmonics=sh, opacities=opac, scales=sc, rotations=rot)


ADAPTER_OUTPUTS = ("means", "covariances", "harmonics", "opacities", "scales", "rotations")


@functools.lru_cache(maxsize=None)
def _adapter_table(sh_degree, pad):
    """67 rows; every row belongs to one density group and one quaternion group, every scale logit to one softplus group; the three
    assignments are balanced and shuffled independently, so the groups meet in many combinations."""
    g = torch.Generator().manual_seed(700 + 10 * sh_degree + pad)
    U, dsh = ADAPTER_ROWS, (sh_degree + 1) ** 2
    feats = torch.full((U, 8 + 3 * dsh + pad), NAN)
    di, qi, si = _balanced(U, len(DENSITY_X), g), _balanced(U, len(QUAT_GROUPS), g), _balanced(3 * U, len(SOFTPLUS_X), g).view(U, 3)
    feats[:, 0] = torch.tensor(DENSITY_X)[di]
    feats[:, 1:4] = torch.tensor(SOFTPLUS_X)[si]
    base = torch.nn.functional.normalize(torch.randn(U, 4, generator=g, dtype=F64), dim=-1)
    for r in range(U):
        name = QUAT_GROUPS[int(qi[r])]
        q = base[r] * QUAT_SCALE[name]
        if name == "single":
            q = torch.zeros(4, dtype=F64)
            q[r % 4] = 0.7 if r % 8 < 4 else -0.7
        elif name == "negw":
            q[3] = -(0.3 + q[3].abs())
        feats[r, 4:8] = q.float()
    feats[:, 8:8 + 3 * dsh] = torch.randn(U, 3 * dsh, generator=g)
    pts = torch.randn(U, 3, generator=g) * 2
    return pts, feats, di, qi, si


def adapter_case(sh_degree, U, pad, op_exp):
    """The 67-row table of this degree, handed to the kernel U rows per launch (the last launch ragged): every row takes its
    branches at every launch size.  U = 1 / 3 / 4 / 5 leave 16-lane groups and waves partly idle, 67 fills one workgroup and 3/16
    of the next."""
    pts, feats, di, qi, si = _adapter_table(sh_degree, pad)
    return dict(name=f"adapter[deg{sh_degree},U{U},pad{pad},exp{op_exp}]", pts=pts, feats=feats, sh_degree=sh_degree, U=U, pad=pad,
                op_exp=op_exp, groups=dict(density=di, quat=qi, softplus=si))


def adapter_census(case):
    """group sizes from the inputs alone, and the branch each group is meant to take from the fp64 oracle's intermediate values"""
    f = case["feats"].double()
    x, q = f[:, 1:4], f[:, 4:8]
    n = q.norm(dim=-1)
    sp = 0.001 * softplus(x)
    c = dict(softplus={v: int((x == v).sum()) for v in SOFTPLUS_X}, density={v: int((f[:, 0] == v).sum()) for v in DENSITY_X})
    c["passthrough"] = int((x > 20).sum())
    c["capped"] = int((sp >= 0.3).sum())
    c["exp_underflows"] = int((x <= -104).sum())
    c["quat"] = dict(unit=int(((n - 1).abs() < 1e-6).sum()),
                     small=int(((n / 1e-3 - 1).abs() < 1e-6).sum()), large=int(((n / 1e3 - 1).abs() < 1e-6).sum()),
                     tiny=int(((n / 1e-12 - 1).abs() < 1e-6).sum()), single=int(((q != 0).sum(-1) == 1).sum()),
                     negw=int(((q[:, 3] < 0) & (n > 1 + 1e-3) & (n < 2)).sum()))
    c["negative_w_rows"] = int((q[:, 3] < 0).sum())
    c["zero_quat"] = int((n == 0).sum())
    # (-104, -87) is where fp32 exp is subnormal; the arguments are x (softplus) and -logit (sigmoid; its result 1 + exp is 1 there)
    c["subnormal_exp_args"] = int(((x > -104) & (x < -87)).sum())
    return c


def adapter_saturation_case(op_exp):
    """all-zero quaternions, quaternions scaled by 1e25 (the squared norm overflows fp32) and density logits of +-100, four rows each"""
    g = torch.Generator().manual_seed(733)
    deg, U = 1, 16
    feats = torch.randn(U, 8 + 3 * 4, generator=g)
    feats[:, 4:8] = torch.nn.functional.normalize(feats[:, 4:8], dim=-1)
    feats[0:4, 4:8] = 0.0
    feats[4:8, 4:8] *= 1e25
    feats[8:12, 0], feats[12:16, 0] = 100.0, -100.0
    return dict(name=f"adapter_saturation[exp{op_exp}]", pts=torch.randn(U, 3, generator=g), feats=feats, sh_degree=deg, U=U, pad=0,
                op_exp=op_exp)


# ------------------------------------------------------------------------------------------------ depth unprojection
UNPROJECT_SHAPES = ((1, 1, 1), (3, 5, 7), (2, 16, 17), (4, 9, 30))
UNPROJECT_LD = (2, 8)


def unproject_oracle(case, dt, mut=None):
    """raw [S H W, ld] (depth logit, confidence logit), cam [S, 16] = {fx, fy, cx, cy, R^T row-major, -R^T t} ->
    depth [P], conf [P], pts [P, 3].  mut: prev_frame, swap_cxcy, r_for_rt, conf_no_one."""
    S, H, W = case["shape"]
    raw, cam = case["raw"].to(dt), case["cam"].to(dt)
    if mut == "prev_frame":
        cam = cam.roll(1, 0)
    fx, fy, cx, cy = (cam[:, i, None, None] for i in range(4))
    if mut == "swap_cxcy":
        cx, cy = cy, cx
    Rt, tinv = cam[:, 4:13].reshape(S, 3, 3), cam[:, 13:16]
    if mut == "r_for_rt":
        Rt = Rt.transpose(1, 2)
    d = torch.exp(raw[:, 0]).view(S, H, W)
    conf = torch.exp(raw[:, 1]) + (0.0 if mut == "conf_no_one" else 1.0)
    u = torch.arange(W, dtype=dt)[None, None, :]
    v = torch.arange(H, dtype=dt)[None, :, None]
    x = (u - cx) * d / fx
    y = (v - cy) * d / fy
    c = torch.stack((x, y, d), -1).reshape(S, H * W, 3)
    pts = torch.einsum("fij,fpj->fpi", Rt, c) + tinv[:, None, :]
    return dict(depth=d.reshape(-1, 1), conf=conf.reshape(-1, 1), pts=pts.reshape(-1, 3))


UNPROJECT_OUTPUTS = ("depth", "conf", "pts")


def _cameras(S):
    """one distinct, asymmetric camera per frame: fx != fy, cx != cy (neither an integer), a rotation by a large angle about a skew
    axis, a translation of three different components.  -> cam [S, 16] fp32, R [S, 3, 3] and t [S, 3] (fp64 views of fp32 values)"""
    f = torch.arange(S, dtype=F64)
    q = torch.stack([0.5 + 0.1 * f, -0.3 - 0.05 * f, 0.7 - 0.15 * f, 0.4 + 0.02 * f], -1)
    Rm = quat_to_mat(q / q.norm(dim=-1, keepdim=True)).float().double()
    t = torch.stack([0.3 + f, -1.1 - 0.5 * f, 2.2 + 0.25 * f], -1).float().double()
    k = torch.stack([21.0 + 3.0 * f, 28.5 + 4.0 * f, 3.37 + 0.5 * f, 2.29 - 0.3 * f], -1)
    Rt = Rm.transpose(1, 2)
    tinv = -(Rt @ t[:, :, None])[:, :, 0]
    return torch.cat([k, Rt.reshape(S, 9), tinv], 1).float().contiguous(), Rm, t


def unproject_case(S, H, W, ld):
    g = torch.Generator().manual_seed(800 + 97 * S + 13 * H + W + ld)
    raw = torch.full((S * H * W, ld), NAN)
    raw[:, :2] = torch.rand(S * H * W, 2, generator=g) * 6 - 3
    if S * H * W == 1:
        # One pixel is one draw of the fp32 rounding error from [0, 1/2 ulp]; a draw near 0 would turn 4 x e32 into bit equality with
        # the fp64 value, which no fp32 evaluation promises.  These two logits were picked on the CPU, from the fp32 oracle alone, as
        # a pair whose three outputs each miss fp64 by a quarter ulp or more (depth 3.1e-8, conf 4.6e-8, pts 7.4e-8).
        raw[0, 0], raw[0, 1] = 1.9, -1.3
    cam, Rm, t = _cameras(S)
    return dict(name=f"unproject[{S}x{H}x{W},ld{ld}]", raw=raw, cam=cam, shape=(S, H, W), ld=ld, R=Rm, t=t)


def unproject_census(case):
    S, H, W = case["shape"]
    P = S * H * W
    frame = torch.arange(P) // (H * W)
    block = torch.arange(P) // 256
    straddling = sum(int(frame[block == b].unique().numel() > 1) for b in range((P + 255) // 256))
    cam, Rm = case["cam"].double(), case["R"]
    asym = (Rm - Rm.transpose(1, 2)).flatten(1).norm(dim=1)
    return dict(frame=frame, per_frame=[int((frame == f).sum()) for f in range(S)], straddling_blocks=straddling,
                fx_ne_fy=bool((cam[:, 0] != cam[:, 1]).all()), cx_ne_cy=bool((cam[:, 2] != cam[:, 3]).all()),
                cameras_distinct=len({tuple(r.tolist()) for r in cam}) == S, min_asymmetry=float(asym.min()),
                t_components_differ=bool(all(len(set(r.tolist())) == 3 for r in case["t"])),
                raw_min=float(case["raw"][:, :2].min()), raw_max=float(case["raw"][:, :2].max()))


def unproject_saturation_case():
    """raw values of +100 (exp overflows fp32) and -110 (exp is zero) in both columns, in all four combinations, four pixels each"""
    S, H, W = 2, 4, 5
    c = unproject_case(S, H, W, 2)
    raw = c["raw"]
    for i, (a, b) in enumerate(((100.0, None), (-110.0, None), (None, 100.0), (None, -110.0), (100.0, 100.0), (-110.0, -110.0),
                                (100.0, -110.0), (-110.0, 100.0))):
        for j in range(4):
            p = (i * 4 + j) * 5 % (S * H * W)     # spread over both frames and all columns
            if a is not None:
                raw[p, 0] = a
            if b is not None:
                raw[p, 1] = b
    return dict(c, name="unproject_saturation")


# ------------------------------------------------------------------------------------------------ bilinear resize
BILINEAR_SHAPES = (((4, 6), (8, 12)), ((5, 5), (5, 5)), ((3, 4), (7, 9)), ((7, 9), (3, 4)), ((1, 5), (4, 5)), ((5, 1), (5, 3)),
                   ((6, 6), (1, 1)))
BILINEAR_EXACT = (((4, 6), (8, 12)), ((5, 5), (5, 5)))        # dyadic inputs; bit-equal where the weights are dyadic too
BILINEAR_FLAGS = tuple((a, t, r) for a in (False, True) for t in (False, True) for r in (False, True))
BILINEAR_TC = ((1, 8), (3, 24), (1, 24), (3, 8))


def _src(o_n, i_n, align, dt, no_zero_clamp=False):
    """source coordinate of every output index along one axis, F.interpolate's rule"""
    o = torch.arange(o_n, dtype=dt)
    if align:
        if o_n == 1:
            return torch.zeros(1, dtype=dt)
        return torch.tensor(float(i_n - 1), dtype=dt) / torch.tensor(float(o_n - 1), dtype=dt) * o
    scale = torch.tensor(float(i_n), dtype=dt) / torch.tensor(float(o_n), dtype=dt)
    s = (o + 0.5) * scale - 0.5
    return s if no_zero_clamp else s.clamp_min(0.0)


def bilinear_oracle(case, dt, mut=None):
    """x [T, h, w, C] bf16 -> [T, H, W, C] (+ add bf16 [T, H, W, C]) (+ table f32 [H W, C], the same for every t) (ReLU last).
    mut: swap_align, no_hi_clamp (x1 / y1 = x0 / y0 + 1 whatever the edge: reads the next row, frame, or beyond), no_zero_clamp
    (negative source coordinate kept, truncated towards zero as a float -> int cast does), relu_first (ReLU before the addends)."""
    x = case["x"].to(dt)
    T, h, w, C = x.shape
    H, W = case["size"]
    align = case["align"] != (mut == "swap_align")
    sy, sx = (_src(o, i, align, dt, mut == "no_zero_clamp") for o, i in ((H, h), (W, w)))
    y0, x0 = sy.trunc().long(), sx.trunc().long()
    ly, lx = (sy - y0.to(dt))[None, :, None, None], (sx - x0.to(dt))[None, None, :, None]
    if mut == "no_hi_clamp":       # the flat buffer as the kernel would walk it, with something conspicuous behind its end
        flat = torch.cat([x.reshape(-1, C), torch.full((h * w + w + 2, C), 100.0, dtype=dt)])
        base = (torch.arange(T) * h * w)[:, None, None]
        at = lambda yy, xx: flat[base + yy[None, :, None] * w + xx[None, None, :]]
        a, b, c, d = at(y0, x0), at(y0, x0 + 1), at(y0 + 1, x0), at(y0 + 1, x0 + 1)
    else:
        y1, x1 = (y0 + 1).clamp_max(h - 1), (x0 + 1).clamp_max(w - 1)
        a, b, c, d = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    hy, hx = 1 - ly, 1 - lx
    o = hy * (hx * a + lx * b) + ly * (hx * c + lx * d)
    if mut == "relu_first" and case["relu"]:
        o = o.clamp_min(0.0)
    if case["add"] is not None:
        o = o + case["add"].to(dt)
    if case["table"] is not None:
        o = o + case["table"].to(dt).view(1, H, W, C)
    if case["relu"] and mut != "relu_first":
        o = o.clamp_min(0.0)
    return o


def bilinear_case(hw, HW, align, T, C, add, table, relu):
    (h, w), (H, W) = hw, HW
    g = torch.Generator().manual_seed(900 + 31 * h + 17 * w + 7 * H + 3 * W + 2 * align + T + C + 64 * add + 128 * table + 256 * relu)
    exact = (hw, HW) in BILINEAR_EXACT
    mk = (lambda *s: grid(s, g, 2.0 ** -4)) if exact else (lambda *s: torch.randn(*s, generator=g) * 1.5)
    return dict(name=f"bilinear[{h}x{w}->{H}x{W},align{int(align)},T{T},C{C},add{int(add)},table{int(table)},relu{int(relu)}]",
                x=mk(T, h, w, C).to(BF16), size=(H, W), align=align, add=mk(T, H, W, C).to(BF16) if add else None,
                table=mk(H * W, C) if table else None, relu=relu, exact=exact)


def _axis_census(o_n, i_n, align):
    """(indices whose source index is the last one, indices clamped at 0, last-index hits with a non-zero weight on the neighbour
    that must be clamped), in exact integer arithmetic"""
    last, zero, last_frac = [], [], []
    for o in range(o_n):
        if align:
            num, den = ((i_n - 1) * o, o_n - 1) if o_n > 1 else (0, 1)            # src = num / den
        else:
            num, den = (2 * o + 1) * i_n - o_n, 2 * o_n                          # src = (o + .5) i / O - .5
            if num < 0:
                zero.append(o)
                num = 0
        if num // den == i_n - 1:
            last.append(o)
            if num % den:
                last_frac.append(o)
    return last, zero, last_frac


def bilinear_census(case):
    """output pixels (t, oy, ox) whose y0 or x0 is the source's last row / column, and those whose coordinate was clamped at 0"""
    T, h, w, _ = case["x"].shape
    H, W = case["size"]
    (ly, zy, fy), (lx, zx, fx) = _axis_census(H, h, case["align"]), _axis_census(W, w, case["align"])
    union = lambda ys, xs: T * (len(ys) * W + len(xs) * H - len(ys) * len(xs))
    return dict(last=union(ly, lx), clamped0=union(zy, zx), last_with_weight=union(fy, fx), last_y=ly, last_x=lx, zero_y=zy, zero_x=zx)


# ------------------------------------------------------------------------------------------------ temporal upsample
UPT_CASES = tuple((Tl, C, hw) for Tl in (1, 2, 4) for C in (8, 16) for hw in ((1, 1), (3, 5)))


def upsample_t_oracle(case, dt, mut=None):
    """z [C, Tl, H, W] -> [4 (Tl - 1) + 1, H, W, C]: linear in t with align_corners=True (weights j / 4).  mut: fifths (weights j / 5),
    swapped (the two weights exchanged), floor (no lerp: the frame below)."""
    z = case["z"].to(dt)
    C, Tl, H, W = z.shape
    T = 4 * (Tl - 1) + 1
    scale = torch.tensor(float(Tl - 1), dtype=dt) / torch.tensor(float(T - 1), dtype=dt) if T > 1 else torch.zeros((), dtype=dt)
    src = scale * torch.arange(T, dtype=dt)
    i0 = src.trunc().long()
    i1 = (i0 + 1).clamp_max(Tl - 1)
    l1 = src - i0.to(dt)
    if mut == "fifths":
        l1 = l1 * 0.8
    elif mut == "floor":
        l1 = l1 * 0
    l0 = 1 - l1
    if mut == "swapped":
        l0, l1 = l1, l0
    o = l0[None, :, None, None] * z[:, i0] + l1[None, :, None, None] * z[:, i1]
    return o.permute(1, 2, 3, 0).contiguous()


def upsample_t_case(Tl, C, hw):
    g = torch.Generator().manual_seed(1000 + 100 * Tl + C + hw[0])
    return dict(name=f"upsample_t[Tl{Tl},C{C},{hw[0]}x{hw[1]}]", z=grid((C, Tl, *hw), g, 2.0 ** -6))


def upsample_t_census(case):
    Tl = case["z"].shape[1]
    T = 4 * (Tl - 1) + 1
    return dict(frames=T, copied=[t for t in range(T) if t % 4 == 0], blended=[t for t in range(T) if t % 4], last_clamped=[T - 1])


# ------------------------------------------------------------------------------------------------ fp32 skinny linear
#                (M, N, K, act, gamma + residual, kind): every M in 1 / 16 / 17 / 32, N in 1 / 5 / 9 / 33, K in 4 / 12 / 256 / 260 / 508
LINEAR_CASES = ((1, 1, 4, "none", False, "dyadic"), (16, 5, 12, "gelu", True, "randn"), (17, 9, 260, "silu", False, "randn"),
                (32, 33, 508, "relu", True, "randn"), (17, 33, 256, "none", True, "randn"), (16, 9, 508, "gelu", False, "randn"),
                (32, 5, 260, "silu", True, "randn"), (1, 33, 12, "relu", False, "randn"),
                (17, 9, 260, "none", False, "tail"), (32, 33, 508, "none", True, "tail"), (16, 5, 260, "none", False, "tail"),
                # N above 1024, where the host first gives a wave more than one output (linear_npw): <32,2> with the last live wave
                # half valid, <16,2> the same with tail values, <16,3> with one of a wave's three outputs dropped
                (32, 1029, 12, "none", False, "randn"), (16, 1027, 260, "none", False, "tail"), (16, 2999, 12, "silu", True, "randn"))
ACTS = dict(none=lambda t: t, gelu=torch.nn.functional.gelu, silu=torch.nn.functional.silu, relu=torch.relu)


def linear_oracle(case, dt, mut=None):
    """y = act(x W^T + b) (x gamma) (+ residual).  mut: drop_last4 (the last four k left out), twice_last4 (counted twice),
    gamma_last (gamma applied after the residual), no_bias."""
    x, w = case["x"].to(dt), case["w"].to(dt)
    y = x @ w.t()
    if mut in ("drop_last4", "twice_last4"):
        y = y + (-1 if mut == "drop_last4" else 1) * (x[:, -4:] @ w[:, -4:].t())
    if mut != "no_bias":
        y = y + case["b"].to(dt)
    y = ACTS[case["act"]](y)
    if case["gamma"] is not None:
        if mut == "gamma_last":
            return (y + case["res"].to(dt)) * case["gamma"].to(dt)
        y = y * case["gamma"].to(dt) + case["res"].to(dt)
    return y


def linear_case(M, N, K, act, extra, kind):
    """kind: randn; dyadic (multiples of 1/8: every product and sum is exact in fp32, so the one output must be bit-equal); tail (1e6 in
    the last four floats of every x and w row: an output is 4e12 + O(sqrt K), and a lane that uses a re-read tail adds 4e12 more)"""
    g = torch.Generator().manual_seed(1100 + 64 * M + 8 * N + K + len(act))
    if kind == "dyadic":
        x, w, b = grid((M, K), g, 0.125), grid((N, K), g, 0.125), grid((N,), g, 0.125)
    else:
        x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g) * 0.1
    if kind == "tail":
        x[:, -4:], w[:, -4:] = 1e6, 1e6
    res = torch.randn(M, N, generator=g) if extra else None
    gam = 0.3 * (1 + 0.2 * torch.randn(N, generator=g)) if extra else None
    return dict(name=f"linear[M{M},N{N},K{K},{act},ls{int(extra)},{kind}]", x=x, w=w, b=b, res=res, gamma=gam, act=act, kind=kind)


def linear_npw(M, N):
    """the host's choice of outputs per wave (v3a_linear_f32): the count, up to 4 (2 above 16 rows), whose workgroups of four waves
    come closest to whole rounds of 256; ties go to the larger count"""
    best, beff = 1, -1.0
    for npw in range(1, (4 if M <= 16 else 2) + 1):
        wgs = (N + 4 * npw - 1) // (4 * npw)
        eff = wgs / ((wgs + 255) // 256 * 256)
        if eff >= beff - 1e-9:
            best, beff = npw, eff
    return best


def linear_census(case):
    """The kernel instantiation <rows held per lane, outputs per wave> that THIS case launches (the host's choice replayed), and what
    its waves do: idle (first output >= N: stages and waits, computes clamped rows, stores nothing), partly valid (some outputs
    < N, some >= N: the clamped weight row is computed and dropped), how many outputs are dropped in partly valid waves; and what
    the last 256-wide chunk of K looks like."""
    (M, K), N = case["x"].shape, case["w"].shape[0]
    npw = linear_npw(M, N)
    wgs = (N + 4 * npw - 1) // (4 * npw)
    first = [wv * npw for wv in range(4 * wgs)]
    partly = [n0 for n0 in first if n0 < N < n0 + npw]
    last = K - (K - 1) // 256 * 256
    return dict(instantiation=(16 if M <= 16 else 32, npw), workgroups=wgs, idle_waves=sum(n0 >= N for n0 in first),
                partly_valid_waves=len(partly), dropped_in_partly_valid=sum(n0 + npw - N for n0 in partly),
                chunks=(K + 255) // 256, last_chunk_floats=last, rereading_lanes=64 - last // 4)


# ------------------------------------------------------------------------------------------------ fp32 small attention
ATTENTION_CASES = ((1, 1, 128, 1.0), (2, 3, 8, 1.0), (13, 2, 32, 1.0), (64, 1, 64, 1.0), (33, 4, 128, 1.0), (13, 2, 32, 40.0))


def attention_oracle(case, dt, mut=None):
    """qkv [S, 3 H hd] -> [S, H hd], softmax(q k^T hd^-1/2) v per head.  mut: scale_inv_hd, kv_swapped, softmax_over_queries."""
    qkv, H = case["qkv"].to(dt), case["H"]
    S = qkv.shape[0]
    hd = qkv.shape[1] // (3 * H)
    q, k, v = qkv.view(S, 3, H, hd).permute(1, 2, 0, 3)
    if mut == "kv_swapped":
        k, v = v, k
    s = q @ k.transpose(-1, -2) * (1.0 / hd if mut == "scale_inv_hd" else hd ** -0.5)
    dim = -2 if mut == "softmax_over_queries" else -1
    e = torch.exp(s - s.amax(dim, keepdim=True))
    p = e / e.sum(dim, keepdim=True)
    return (p @ v).permute(1, 0, 2).reshape(S, H * hd)


def attention_case(S, H, hd, spread):
    """spread > 1: query i is `spread` times the direction of key (5 i + 1) % S, so that key scores +spread, its negated twin key
    scores -spread, and the others lie in between: one key holds the whole softmax"""
    g = torch.Generator().manual_seed(1200 + 100 * S + 10 * H + hd + int(spread))
    qkv = torch.randn(S, 3, H, hd, generator=g)
    if spread > 1:
        k = torch.nn.functional.normalize(torch.randn(S, H, hd, generator=g, dtype=F64), dim=-1)
        k[1::2] = -k[0:S - 1:2]                                     # twins: key 2 j + 1 = -key 2 j
        q = k[(5 * torch.arange(S) + 1) % S] * spread * math.sqrt(hd)
        qkv[:, 0], qkv[:, 1] = q.float(), k.float()
    return dict(name=f"attention[S{S},H{H},hd{hd},spread{spread:g}]", qkv=qkv.reshape(S, 3 * H * hd).contiguous(), H=H, hd=hd, spread=spread)


def attention_census(case):
    qkv, H = case["qkv"].double(), case["H"]
    S, hd = qkv.shape[0], case["hd"]
    q, k, _ = qkv.view(S, 3, H, hd).permute(1, 2, 0, 3)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    p = torch.softmax(s, -1)
    return dict(rows=S * H, max_score=float(s.max()), min_score=float(s.min()), dominated_rows=int((p.amax(-1) > 0.999).sum()),
                idle_pv_lanes=max(0, 64 - hd), idle_score_lanes=64 - S)


# ------------------------------------------------------------------------------------------------ all cases, all mutants
def adapter_cases():
    return [adapter_case(d, U, pad, e) for d in range(5) for U in ADAPTER_U for pad in ADAPTER_PAD for e in ADAPTER_EXP]


def unproject_cases():
    return [unproject_case(*s, ld) for s in UNPROJECT_SHAPES for ld in UNPROJECT_LD]


def bilinear_cases(hw, HW, align):
    i0 = BILINEAR_SHAPES.index((hw, HW)) + int(align)
    return [bilinear_case(hw, HW, align, *BILINEAR_TC[(i0 + i) % 4], *f) for i, f in enumerate(BILINEAR_FLAGS)]


def all_bilinear_cases():
    return [c for hw, HW in BILINEAR_SHAPES for align in (False, True) for c in bilinear_cases(hw, HW, align)]


def upsample_t_cases():
    return [upsample_t_case(*c) for c in UPT_CASES]


def linear_cases():
    return [linear_case(*c) for c in LINEAR_CASES]


def attention_cases():
    return [attention_case(*c) for c in ATTENTION_CASES]


def _rows(t):
    """[rows, row elements] of an output whose last dim is the row (a pixel's channels, an output row, a Gaussian's values)"""
    return t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(-1, 1)


def as_rows(kernel, out):
    """dict output name -> [rows, ...] for the metric"""
    if kernel == "adapter":
        return {n: out[n].reshape(out[n].shape[0], -1) for n in ADAPTER_OUTPUTS}
    if kernel == "unproject":
        return {n: out[n] for n in UNPROJECT_OUTPUTS}
    if kernel == "upsample_t":                  # judged in the kernel's output format
        out = out.to(BF16)
    return dict(out=_rows(out))


ORACLES = dict(adapter=adapter_oracle, unproject=unproject_oracle, bilinear=bilinear_oracle, upsample_t=upsample_t_oracle,
               linear=linear_oracle, attention=attention_oracle)


def reference(kernel, case, keep=None):
    """(fp64 rows, e32 per output, gate per output) of a case; keep: output name -> bool [rows], the rows that count (saturation)"""
    r64 = as_rows(kernel, ORACLES[kernel](case, F64))
    r32 = as_rows(kernel, ORACLES[kernel](case, F32))
    e32 = {n: per_row_error(r32[n], r64[n], None if keep is None else keep[n]) for n in r64}
    return r64, e32, {n: gate_from(e) for n, e in e32.items()}


# mutant -> the cases it concerns (a rule that a case never exercises cannot be seen there)
MUTANTS = dict(
    adapter=dict(no_threshold=lambda c: True, no_cap=lambda c: True, exp_one=lambda c: c["op_exp"] != 1.0, wxyz=lambda c: True),
    unproject=dict(prev_frame=lambda c: c["shape"][0] > 1, swap_cxcy=lambda c: True, r_for_rt=lambda c: True, conf_no_one=lambda c: True),
    bilinear=dict(swap_align=lambda c: min(c["x"].shape[1:3]) > 1 and tuple(c["x"].shape[1:3]) != c["size"],
                  no_hi_clamp=lambda c: bilinear_census(c)["last_with_weight"] > 0,
                  no_zero_clamp=lambda c: bool(bilinear_census(c)["zero_y"] and c["x"].shape[1] > 1 or bilinear_census(c)["zero_x"] and c["x"].shape[2] > 1),
                  relu_first=lambda c: c["relu"] and (c["add"] is not None or c["table"] is not None)),
    upsample_t=dict(fifths=lambda c: c["z"].shape[1] > 1, swapped=lambda c: c["z"].shape[1] > 1, floor=lambda c: c["z"].shape[1] > 1),
    linear=dict(drop_last4=lambda c: True, twice_last4=lambda c: True, gamma_last=lambda c: c["gamma"] is not None and c["kind"] == "randn", no_bias=lambda c: c["kind"] == "randn"),
    attention=dict(scale_inv_hd=lambda c: c["qkv"].shape[0] > 1, kv_swapped=lambda c: True, softmax_over_queries=lambda c: c["qkv"].shape[0] > 1 and c["spread"] == 1))
