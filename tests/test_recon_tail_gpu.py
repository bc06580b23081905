"""The six small kernels of the reconstruction tail on the GPU: every case of tests/recon_tail_cases.py through its `ops` wrapper,
every row (a Gaussian, a pixel, an output row) judged on its own against the fp64 restatement of the operation.
tests/test_recon_tail_host.py shows, without a GPU, that the restatements are the reconstruction oracle's formulas, that each case
takes the branches it was built for, and that a restatement with one rule changed misses these gates by more than 10x.

Metric: max over rows of ||hip - ref64|| / (||ref64|| + floor), floor = 1e-3 x the median non-zero row norm.  Nothing excused.
Gate, formed at run time per case and output: min(4 x e32, 1e-3), e32 = the fp32 CPU run of the same restatement against its fp64
run on the same metric (the 4x covers the device's exp / log1p / pow / erf and another summation order).  e32 = 0 means the case
is exact in fp32: the gate is then bit equality with the fp64 value.  bf16 outputs: the temporal upsample is exact before its
rounding, so it must equal bf16(ref64) bit for bit; a bf16 bilinear output must equal the bf16 rounding of the same call's fp32 output.
Every call is made twice and must return the same bits.  Padding: the `ops` wrappers allocate every output densely and at its exact
size, so a call made through them has no unused output region to fill with a sentinel; writes beyond an output are the business of
tests/test_guard_bands_gpu.py, which calls the C ABI with over-allocated buffers.  What is checked here is the input side: the padding
columns of the strided inputs (feats with ldf > 8 + 3 dsh, raw with ld = 8) hold NaN, no NaN may reach any output (nobody read
them), and the inputs come back bit for bit as they went in.

Saturation cases (all-zero and 1e25-scaled quaternions, density logits of +-100, depth / confidence logits of +100 and -110) are
judged against the fp32 CPU run of the restatement: the same class (finite, +inf, -inf, NaN) element by element; rows that are
finite there but far from fp64 (a quaternion over an infinite norm is 0, exp(-110) is 0: exact operands, nothing rounded) must hold
the fp32 oracle's very values; the remaining finite rows go by the metric and gate above.

Measured on an MI355X (hip vs fp64 | fp32 oracle vs fp64, ranges over the cases; the gate is 4 x the second figure of the same case;
worst hip / gate over all cases in brackets):
  gaussian_adapter (150)   covariances 3.2e-7 .. 5.7e-7 | 3.5e-7 .. 5.6e-7 [0.35]   rotations 1.1e-7 .. 1.5e-7 | 8.6e-8 .. 1.0e-7 [0.39]
                           scales 8.3e-8 | 8.3e-8 [0.25]   opacities 2.1e-6 .. 2.3e-5 | the same [0.25]   harmonics <= 1.3e-8 | the same
                           [0.25], bit-equal at degree 0   means bit-equal
  depth_unproject (8)      depth 3.1e-8 .. 7.5e-8 | 3.1e-8 .. 5.8e-8 [0.33]   conf 4.6e-8 .. 9.0e-8 | 4.6e-8 .. 8.7e-8 [0.27]
                           pts 7.4e-8 .. 2.2e-7 | 7.4e-8 .. 2.4e-7 [0.28]
  bilinear_cl (112)        <= 4.5e-6 | <= 5.0e-6 [0.26]; 48 cases bit-equal (gate 0)       latent_upsample_t_cl (12)  all bit-equal
  linear_f32 (14)          <= 3.2e-7 | <= 3.9e-7 [0.27]; the dyadic case bit-equal; the instantiations with several outputs per wave and
                           a dropped output: <32,2> N = 1029 6.4e-8 | 8.6e-8, <16,2> N = 1027 (1e6 tails) 4.1e-9 | 4.1e-9, <16,3> N = 2999
                           3.6e-8 | 3.6e-8
  attention_small_f32 (6)  <= 5.8e-7 | <= 5.3e-7 [0.27]; S = 1 bit-equal
  saturation               every class as the fp32 oracle's; ordinary rows: covariances 3.5e-7, scales 1.2e-7, pts 1.3e-7 [<= 0.25]"""
import pytest
import torch

import recon_tail_cases as T

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _judge(parity, kernel, case, got, keep=None):
    """print every figure beside the fp32 oracle's, log it, then assert all of them.  got: output name -> [rows, ...]"""
    r64, e32, gate = T.reference(kernel, case, keep)
    bad = []
    for n in r64:
        e = T.per_row_error(got[n], r64[n], None if keep is None else keep[n])
        print(f"[{case['name']}] {n}: hip vs fp64 {e:.3e}   oracle fp32 vs fp64 {e32[n]:.3e}   gate {gate[n]:.3e}")
        parity(f"recon_tail::{case['name']}", output=n, metric="per_row_max", hip=e, oracle_fp32=e32[n], gate=gate[n])
        if not T.passes(e, gate[n]):
            bad.append((n, e, e32[n], gate[n]))
    assert not bad, (case["name"], bad)


def _twice(fn):
    """the call's outputs (a dict of tensors), made twice: the same bits both times"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for n in a:
        assert _same_bits(a[n], b[n]), n
    return a


def _judge_saturation(parity, kernel, case, got):
    """classes as the fp32 oracle's everywhere, its values in the saturated finite rows, the fp64 metric in the ordinary ones"""
    ref32 = T.as_rows(kernel, T.ORACLES[kernel](case, F32))
    ref64 = T.as_rows(kernel, T.ORACLES[kernel](case, F64))
    _same_classes(case, got, ref32)
    keep = {}
    for n in ref32:
        keep[n], sat = T.saturation_split(ref32[n], ref64[n])
        print(f"[{case['name']}] {n}: {int(keep[n].sum())} ordinary rows, {int(sat.sum())} saturated finite rows, "
              f"{int((~torch.isfinite(ref32[n]).all(1)).sum())} non-finite rows")
        assert torch.equal(got[n][sat], ref32[n][sat]), (case["name"], n)
    _judge(parity, kernel, case, got, keep=keep)


def _same_classes(case, got, ref32):
    bad = {n: int((T.value_class(got[n]) != T.value_class(ref32[n])).sum()) for n in ref32}
    print(f"[{case['name']}] elements of another class than the fp32 oracle's: {bad}; "
          f"non-finite in the oracle: { {n: int((T.value_class(ref32[n]) != 0).sum()) for n in ref32} }")
    assert not any(bad.values()), (case["name"], bad)


# ------------------------------------------------------------------------------------------------ gaussian adapter
def _run_adapter(ops, case):
    """the table through the kernel, U rows per launch, on row slices of the strided feature matrix"""
    deg = case["sh_degree"]
    pts, feats = case["pts"].cuda(), case["feats"].cuda()
    before = feats.clone()
    mask = T.R.sh_mask(deg).cuda()
    n, U = feats.shape[0], case["U"]

    def call():
        parts = [ops.gaussian_adapter(pts[r:r + U], feats[r:r + U], mask, sh_degree=deg, opacity_exponent=case["op_exp"]) for r in range(0, n, U)]
        return {k: torch.cat([p[k] for p in parts]) for k in T.ADAPTER_OUTPUTS}
    out = _twice(call)
    assert _same_bits(feats, before)                      # the NaN padding behind every row included
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("U", T.ADAPTER_U)
@pytest.mark.parametrize("deg", range(5))
def test_gaussian_adapter_branches_per_gaussian(hip_lib, parity, deg, U):
    from vist3a_amd import ops
    for pad in T.ADAPTER_PAD:
        for e in T.ADAPTER_EXP:
            case = T.adapter_case(deg, U, pad, e)
            out = _run_adapter(ops, case)
            assert not any(bool(torch.isnan(v).any()) for v in out.values()), case["name"]     # nobody read the padding
            assert torch.equal(out["means"], case["pts"])
            _judge(parity, "adapter", case, T.as_rows("adapter", out))


@pytest.mark.parametrize("op_exp", T.ADAPTER_EXP)
def test_gaussian_adapter_saturation_follows_the_reference_formulas(hip_lib, parity, op_exp):
    from vist3a_amd import ops
    case = T.adapter_saturation_case(op_exp)
    _judge_saturation(parity, "adapter", case, T.as_rows("adapter", _run_adapter(ops, case)))


# ------------------------------------------------------------------------------------------------ depth unprojection
def _run_unproject(ops, case):
    S, H, W = case["shape"]
    raw, cam = case["raw"].cuda(), case["cam"].cuda()
    before = raw.clone()
    out = _twice(lambda: dict(zip(T.UNPROJECT_OUTPUTS, ops.depth_unproject(raw, cam, S, H, W))))
    assert _same_bits(raw, before)
    assert out["depth"].shape == (S, H, W) and out["conf"].shape == (S, H, W) and out["pts"].shape == (S, H, W, 3)
    return dict(depth=out["depth"].cpu().reshape(-1, 1), conf=out["conf"].cpu().reshape(-1, 1), pts=out["pts"].cpu().reshape(-1, 3))


@pytest.mark.parametrize("ld", T.UNPROJECT_LD)
@pytest.mark.parametrize("S,H,W", T.UNPROJECT_SHAPES)
def test_depth_unproject_per_pixel(hip_lib, parity, S, H, W, ld):
    from vist3a_amd import ops
    case = T.unproject_case(S, H, W, ld)
    _judge(parity, "unproject", case, _run_unproject(ops, case))


def test_depth_unproject_saturation_follows_the_reference_formulas(hip_lib, parity):
    from vist3a_amd import ops
    case = T.unproject_saturation_case()
    _judge_saturation(parity, "unproject", case, _run_unproject(ops, case))


# ------------------------------------------------------------------------------------------------ bilinear resize
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("hw,HW", T.BILINEAR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bilinear_cl_per_pixel(hip_lib, parity, hw, HW, align):
    from vist3a_amd import ops
    for case in T.bilinear_cases(hw, HW, align):
        x = case["x"].cuda()
        add = case["add"].cuda() if case["add"] is not None else None
        tab = case["table"].cuda() if case["table"] is not None else None
        kw = dict(align_corners=align, add=add, table=tab, relu=case["relu"])
        out = _twice(lambda: dict(f32=ops.bilinear_cl(x, HW, out_f32=True, **kw), bf16=ops.bilinear_cl(x, HW, out_f32=False, **kw)))
        assert out["f32"].dtype == F32 and out["bf16"].dtype == BF16 and out["f32"].shape == (x.shape[0], *HW, x.shape[3])
        assert _same_bits(out["bf16"], out["f32"].to(BF16)), case["name"]
        if hw == HW and add is None and tab is None:      # the identity resize of any finite input is that input
            assert torch.equal(out["f32"], x.float().relu() if case["relu"] else x.float()), case["name"]
        _judge(parity, "bilinear", case, T.as_rows("bilinear", out["f32"].cpu()))


# ------------------------------------------------------------------------------------------------ temporal upsample
@pytest.mark.parametrize("Tl,C,hw", T.UPT_CASES, ids=lambda s: str(s).replace(" ", ""))
def test_latent_upsample_t_is_exact(hip_lib, parity, Tl, C, hw):
    from vist3a_amd import ops
    case = T.upsample_t_case(Tl, C, hw)
    z = case["z"].cuda()
    out = _twice(lambda: dict(out=ops.latent_upsample_t_cl(z)))["out"].cpu()
    assert out.dtype == BF16 and out.shape == (4 * (Tl - 1) + 1, *hw, C)
    for i in range(Tl):                                   # frames with t % 4 == 0 are the latent frames, rounded
        assert _same_bits(out[4 * i], case["z"][:, i].permute(1, 2, 0).to(BF16)), i
    _judge(parity, "upsample_t", case, T.as_rows("upsample_t", out))


# ------------------------------------------------------------------------------------------------ fp32 skinny linear
@pytest.mark.parametrize("spec", T.LINEAR_CASES, ids=lambda s: "-".join(map(str, s)))
def test_linear_f32_per_output_row(hip_lib, parity, spec):
    from vist3a_amd import lib as L
    from vist3a_amd import ops
    case = T.linear_case(*spec)
    d = {k: (case[k].cuda() if case[k] is not None else None) for k in ("x", "w", "b", "res", "gamma")}
    act = dict(none=L.ACT_NONE, gelu=L.ACT_GELU_ERF, silu=L.ACT_SILU, relu=L.ACT_RELU)[case["act"]]
    out = _twice(lambda: dict(out=ops.linear_f32(d["x"], d["w"], d["b"], act=act, residual=d["res"], gamma=d["gamma"])))["out"]
    assert out.shape == (spec[0], spec[1])
    _judge(parity, "linear", case, T.as_rows("linear", out.cpu()))


# ------------------------------------------------------------------------------------------------ fp32 small attention
@pytest.mark.parametrize("spec", T.ATTENTION_CASES, ids=lambda s: "-".join(map(str, s)))
def test_attention_small_f32_per_query_row(hip_lib, parity, spec):
    from vist3a_amd import ops
    case = T.attention_case(*spec)
    qkv = case["qkv"].cuda()
    out = _twice(lambda: dict(out=ops.attention_small_f32(qkv, case["H"])))["out"]
    assert out.shape == (spec[0], spec[1] * spec[2])
    _judge(parity, "attention", case, T.as_rows("attention", out.cpu()))
