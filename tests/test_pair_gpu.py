"""fp32-equivalent ("split bf16") kernels of the DPT heads (include/vist3a_hip.h: v3a_conv_split, v3a_layernorm_pair, v3a_bilinear_cl_pair,
v3a_split_f32) against float64 torch on the CPU.  The bar is `north_star`'s 1e-3 with three decades to spare: the reference runs these
layers in fp32 (autocast off, /root/reference/models/anysplat_stitched.py:335), and a pair carries 16 significand bits, so every kernel must
sit within a few 1e-6 of the exact result - the gates are 2e-5 (measured figures beside each assert) and each test also prints what plain
fp32 torch scores against the same float64 result."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
TOL_SPLIT = 2e-5     # the split-bf16 kernels vs float64 (named so that tests/test_guard_bands_gpu.py applies the same bar; value unchanged)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _pair(x):
    """CPU reference of the pair encoding"""
    hi = x.to(bf16)
    return torch.stack([hi, (x - hi.float()).to(bf16)])


def _cl(x, cp):
    """[T,C,H,W] -> channels-last [T,H,W,cp] zero padded"""
    T, C, H, W = x.shape
    o = torch.zeros(T, H, W, cp, dtype=x.dtype)
    o[..., :C] = x.permute(0, 2, 3, 1)
    return o.contiguous()


def test_split_f32_is_the_pair_encoding(hip_lib):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(4096 * 8, generator=g) * torch.logspace(-20, 20, 4096 * 8)).float()
    x[:8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1e-40, 65504.0])
    p = ops.split_f32(x.cuda()).cpu()
    ref = _pair(x)
    assert torch.equal(p.view(torch.int16), ref.view(torch.int16))
    v = ops.pair_value(p)
    fin = x.abs() > 1e-30
    assert ((v - x).abs()[fin] <= x.abs()[fin] * 2.0 ** -16).all()


@pytest.mark.parametrize("case", ["proj1x1_table", "rcu3x3_res_res2_relu", "down_s2", "upshuffle_rows", "merger7x7_f32out", "narrow_out_f32"])
def test_conv_split_vs_float64(hip_lib, parity, case):
    from vist3a_amd import lib as L
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).float()
    kw, ref_post = {}, None
    T = 2
    if case == "proj1x1_table":
        Cin, Cout, H, W, k = 2048, 256, 32, 32, 1
        table = rn(H * W, Cout, sc=0.1)
        kw = dict(residual=table.cuda(), res_row_mod=H * W)
        ref_post = lambda y: y + table.double().view(1, H, W, Cout).permute(0, 3, 1, 2)
        conv_kw = {}
    elif case == "rcu3x3_res_res2_relu":
        Cin, Cout, H, W, k = 256, 256, 64, 64, 3
        r1, r2 = rn(T, Cout, H, W), rn(T, Cout, H, W)
        kw = dict(pad=(0, 1, 1), residual=_pair(_cl(r1, Cout)).cuda(), residual2=_pair(_cl(r2, Cout)).cuda(), relu_out=True, act=L.ACT_RELU)
        # the pair encoding of the residuals is part of the input: the reference adds exactly what the pairs hold
        r1v, r2v = ops.pair_value(_pair(_cl(r1, Cout))).permute(0, 3, 1, 2).double(), ops.pair_value(_pair(_cl(r2, Cout))).permute(0, 3, 1, 2).double()
        ref_post = lambda y: F.relu(F.relu(y) + r1v + r2v)
        conv_kw = dict(padding=1)
    elif case == "down_s2":
        Cin, Cout, H, W, k = 1024, 1024, 32, 32, 3
        kw = dict(stride=(1, 2, 2), pad=(0, 1, 1))
        conv_kw = dict(stride=2, padding=1)
    elif case == "upshuffle_rows":
        Cin, Cout, H, W, k = 256, 4 * 64, 16, 16, 1     # one dy of a ConvTranspose(k = 4): rows scattered into the 4x taller image
        conv_kw = {}
    elif case == "merger7x7_f32out":
        Cin, Cout, H, W, k = 3, 128, 56, 56, 7
        kw = dict(pad=(0, 3, 3), act=L.ACT_RELU, out_f32=True)
        ref_post = lambda y: F.relu(y)
        conv_kw = dict(padding=3)
    else:
        Cin, Cout, H, W, k = 32, 84, 40, 40, 1
        kw = dict(out_f32=True)
        conv_kw = {}
    x = rn(T, Cin, H, W)
    w = rn(Cout, Cin, k, k, sc=(Cin * k * k) ** -0.5)
    b = rn(Cout, sc=0.1)
    cw = ops.ConvWeightSplit(w, b)
    xp = _pair(_cl(x, cw.CinP))
    xv = ops.pair_value(xp)[..., :Cin].permute(0, 3, 1, 2).double()    # what the pair holds (x to 2^-17) is the input of record
    ref = F.conv2d(xv, w.double(), b.double(), **conv_kw)
    plain = F.conv2d(xv.float(), w, b, **conv_kw).double()
    if ref_post is not None:
        ref = ref_post(ref)
    if case == "upshuffle_rows":
        out = torch.zeros(2, T, H * 4, W, Cout, dtype=bf16).cuda()
        for dy in range(4):
            ops.conv_split(xp.cuda(), cw, out=out, out_rows=(W, 3 * W, dy * W))
        y = ops.pair_value(out).cpu()                    # row (t, 4 h + dy, w) = conv output of pixel (t, h, w), for every dy
        full = ref.permute(0, 2, 3, 1)                   # [T,H,W,Cout]
        for dy in range(4):
            e = _rel(y[:, dy::4], full)
            assert e < TOL_SPLIT, (case, dy, e)
        parity(f"conv_split_{case}", rel=e)
        return
    y = ops.conv_split(xp.cuda(), cw, **kw)
    y = (y if kw.get("out_f32") else ops.pair_value(y)).cpu()[..., :Cout].permute(0, 3, 1, 2)
    e, e32 = _rel(y, ref), _rel(plain if ref_post is None else ref_post(plain), ref)
    parity(f"conv_split_{case}", rel=e, torch_fp32_rel=e32)
    print(f"conv_split {case}: {e:.2e} vs float64 (plain fp32 torch: {e32:.2e})")
    assert e < TOL_SPLIT, (case, e)      # measured <= 6e-6 on MI355X


def test_conv_split_every_tile(hip_lib):
    """every implicit-GEMM tile with a split instantiation gives the same answer to fp32 accumulation-order noise"""
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(5)
    T, Cin, Cout, H, W = 1, 64, 192, 48, 40
    x = torch.randn(T, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (Cin * 9) ** -0.5
    cw = ops.ConvWeightSplit(w, None)
    xp = _pair(_cl(x, Cin))
    ref = F.conv2d(ops.pair_value(xp).permute(0, 3, 1, 2).double(), w.double(), padding=1)
    done = 0
    for tile in range(hip_lib.v3a_gemm_num_tiles()):
        try:
            y = ops.conv_split(xp.cuda(), cw, pad=(0, 1, 1), tile=tile, out_f32=True)
        except RuntimeError:
            continue     # ping-pong tiles have no convolution form
        e = _rel(y.cpu().permute(0, 3, 1, 2), ref)
        assert e < TOL_SPLIT, (tile, e)
        done += 1
    assert done >= 10


def test_conv_split_rejects_what_it_does_not_implement(hip_lib):
    from vist3a_amd import lib as L
    from vist3a_amd import ops
    cw = ops.ConvWeightSplit(torch.randn(16, 16, 1, 1), None)
    xp = torch.zeros(2, 1, 8, 8, 16, dtype=bf16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.conv_split(xp, cw, act=L.ACT_GELU_ERF)


def test_layernorm_pair_vs_float64(hip_lib, parity):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(2)
    for (S, hw, Pp, nsp, d) in ((3, 20, 32, 5, 2048), (2, 9, 16, 5, 128), (1, 7, 8, 1, 520)):
        x = torch.randn(S * Pp, d, generator=g) * 3 + 0.5
        w, b = torch.randn(d, generator=g), torch.randn(d, generator=g)
        y = ops.pair_value(ops.layernorm_pair(x.cuda(), weight=w.cuda(), bias=b.cuda(), eps=1e-5, M=S * hw, in_rows=(hw, Pp - hw, nsp))).cpu()
        xs = x.view(S, Pp, d)[:, nsp:nsp + hw].reshape(S * hw, d).double()
        ref = F.layer_norm(xs, (d,), w.double(), b.double(), 1e-5)
        e = _rel(y, ref)
        parity("layernorm_pair", d=d, rel=e, torch_fp32_rel=_rel(F.layer_norm(xs.float(), (d,), w, b, 1e-5), ref))
        assert e < 1e-5, (d, e)      # measured 4e-6 (the 2^-17 of the stored pair)


def test_bilinear_cl_pair_vs_float64(hip_lib, parity):
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(3)
    for (T, C, h, w, H, W, add, tab) in ((2, 32, 16, 16, 32, 32, False, False), (2, 128, 37, 37, 70, 70, True, True), (1, 256, 8, 8, 16, 16, False, True)):
        x = torch.randn(T, C, h, w, generator=g)
        xp = _pair(_cl(x, C))
        ref = F.interpolate(ops.pair_value(xp).permute(0, 3, 1, 2).double(), size=(H, W), mode="bilinear", align_corners=True)
        kw = {}
        if add:
            a = _pair(_cl(torch.randn(T, C, H, W, generator=g), C))
            kw["add"] = a.cuda()
            ref = ref + ops.pair_value(a).permute(0, 3, 1, 2).double()
        if tab:
            t = torch.randn(H * W, C, generator=g)
            kw["table"] = t.cuda()
            ref = ref + t.double().view(1, H, W, C).permute(0, 3, 1, 2)
        y = ops.pair_value(ops.bilinear_cl_pair(xp.cuda(), (H, W), align_corners=True, **kw)).cpu().permute(0, 3, 1, 2)
        e = _rel(y, ref)
        parity("bilinear_cl_pair", C=C, rel=e)
        assert e < 1e-5, (C, e)


@pytest.mark.parametrize("cout,cin,H,W", [(256, 256, 32, 64), (128, 64, 16, 32), (64, 48, 48, 32), (32, 128, 32, 96), (96, 16, 16, 64)])
def test_conv_split_halo_form_vs_float64(hip_lib, parity, cout, cin, H, W):
    """the halo-tile form (csrc/conv_halo_split.hip), forced with tile=-2: every workgroup width (NJ = 4 / 2 / 1), image borders, several
    tiles per frame, all epilogue operands; against float64 and against the implicit-GEMM form of the same layer"""
    from vist3a_amd import lib as L
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(cout + cin)
    T = 2
    x = torch.randn(T, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (cin * 9) ** -0.5
    b = torch.randn(cout, generator=g) * 0.1
    r1, r2 = _pair(_cl(torch.randn(T, cout, H, W, generator=g), cout)), _pair(_cl(torch.randn(T, cout, H, W, generator=g), cout))
    cw = ops.ConvWeightSplit(w, b)
    assert cw.w_halo is not None
    xp = _pair(_cl(x, cin))
    ref = F.conv2d(ops.pair_value(xp).permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1)
    ref = F.relu(F.relu(ref) + ops.pair_value(r1).permute(0, 3, 1, 2).double() + ops.pair_value(r2).permute(0, 3, 1, 2).double())
    kw = dict(pad=(0, 1, 1), act=L.ACT_RELU, residual=r1.cuda(), residual2=r2.cuda(), relu_out=True)
    yh = ops.pair_value(ops.conv_split(xp.cuda(), cw, tile=-2, **kw)).cpu().permute(0, 3, 1, 2)
    yi = ops.pair_value(ops.conv_split(xp.cuda(), cw, tile=-3, **kw)).cpu().permute(0, 3, 1, 2)
    e, ei, d = _rel(yh, ref), _rel(yi, ref), _rel(yh, yi)
    parity("conv_split_halo", cout=cout, cin=cin, rel=e, implicit_rel=ei, halo_vs_implicit=d)
    print(f"halo split {cin}->{cout} {H}x{W}: {e:.2e} vs float64 (implicit form {ei:.2e}, between them {d:.2e})")
    assert e < TOL_SPLIT and d < 2e-5
    # f32 output + f32 table residual through the same kernel
    tab = torch.randn(H * W, cout, generator=g)
    y32 = ops.conv_split(xp.cuda(), cw, tile=-2, pad=(0, 1, 1), residual=tab.cuda(), res_row_mod=H * W, out_f32=True).cpu().permute(0, 3, 1, 2)
    ref2 = F.conv2d(ops.pair_value(xp).permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1) + tab.double().view(1, H, W, cout).permute(0, 3, 1, 2)
    assert _rel(y32, ref2) < 2e-5


def test_conv_split_halo_not_eligible_is_an_error_when_forced(hip_lib):
    from vist3a_amd import ops
    cw = ops.ConvWeightSplit(torch.randn(32, 16, 3, 3), None)
    xp = torch.zeros(2, 1, 8, 8, 16, dtype=bf16, device="cuda")     # 8 x 8 image: no 16 x 32 tile
    with pytest.raises(RuntimeError):
        ops.conv_split(xp, cw, pad=(0, 1, 1), tile=-2)
    ops.conv_split(xp, cw, pad=(0, 1, 1))                            # automatic: implicit GEMM
