"""GPU: the CLIP score (vist3a_amd.evaluation.clip; csrc/clip.hip + the split GEMMs) against Pillow / transformers for the pixels and
the float64 CPU restatement tests/clip_oracle.py for the towers.

Errors are relative L2 norms against the fp64 oracle (scores: absolute), reported through `parity` and gated at twice the value measured
on an MI355X (MEASURED below, profiles/r7/clip_parity.json).  The fp32 torch oracle sits 2.5e-7 .. 5.4e-7 from
the fp64 one on the same models (tests/test_clip_host.py): attention_f32 is at that level (6.8e-7), every split GEMM and so the towers
are 9 to 19 times above it."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402

SHAPES = [((448, 448), 224), ((448, 448), 378), ((512, 512), 224), ((360, 640), 224), ((301, 517), 224), ((96, 70), 224), ((224, 224), 224)]
FP32_SPREAD = 5.4e-7          # fp32 oracle vs fp64 oracle, tests/test_clip_host.py
# MEASURED: the largest figure each check gave on an MI355X (profiles/r7/clip_parity.json); every gate is twice it.
# The tower figures are 9 to 19 times the fp32 spread: the rounding point is the (hi, lo) bf16 pair itself - 16 significand bits
# (2^-17 per element) at the input of every split GEMM plus its dropped lo x lo product (2^-16) - not any kernel of csrc/clip.hip;
# attention_f32 and the QUICK_GELU epilogue, plain fp32, sit at the fp32 spread.
MEASURED = dict(attention=6.83e-7, quick_gelu=5.18e-6, golden_embed=4.80e-6, golden_hidden=5.59e-6, golden_score=2.13e-4, block=5.86e-6,
                deep_embed=1.035e-5, deep_score=7.12e-5)
GATES = {k: 2 * v for k, v in MEASURED.items()}


def rel(a, b):
    return ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()


def frames_of(H, W, n, seed=0):
    rng = np.random.default_rng(seed + H * 1000 + W)
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        if i % 2:
            out.append(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        else:
            out.append(np.stack([127 + 120 * np.sin(0.05 * (c + 1) * x + 0.03 * y + c + i) for c in range(3)], -1).round().astype(np.uint8))
    return np.stack(out)


class _Pre:
    """just enough of ClipWeights for ClipScorer.preprocess"""
    def __init__(self, S, P):
        from vist3a_amd.evaluation import clip as CL
        self.image_size, self.patch, self.device = S, P, torch.device("cuda")
        self.lut = torch.from_numpy(CL.normalize_lut()).cuda()


@pytest.mark.parametrize("hw,size", SHAPES)
@pytest.mark.parametrize("n", [1, 8])
def test_resize_is_bit_equal_to_pillow_and_transformers(hip_lib, hw, size, n):
    from transformers.image_transforms import normalize, rescale
    from vist3a_amd import ops
    from vist3a_amd.evaluation import clip as CL
    H, W = hw
    P = 14 if size % 14 == 0 else 16
    sc = CL.ClipScorer(_Pre(size, P))
    fr = frames_of(H, W, n)
    patches, u8, pix = sc.preprocess(torch.from_numpy(fr), want_u8=True, want_f32=True)
    oh, ow, top, left = CL.resize_geometry(H, W, size)
    for i in range(n):
        want = np.asarray(Image.fromarray(fr[i]).resize((ow, oh), resample=Image.BICUBIC))[top: top + size, left: left + size]
        assert np.array_equal(u8[i].cpu().numpy(), want), f"frame {i}"
        ref = normalize(rescale(want, 1 / 255, input_data_format="channels_last"), CL.CLIP_MEAN, CL.CLIP_STD,
                        input_data_format="channels_last")
        assert np.array_equal(pix[i].cpu().numpy(), ref.transpose(2, 0, 1)), f"frame {i}: fp32 pixel values differ"   # bit equality
    # the patch matrix is the (hi, lo) split of exactly these values, in the patch convolution's column order, zero padded
    G = size // P
    cols = pix.view(n, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(n * G * G, 3 * P * P)
    hi = cols.to(torch.bfloat16)
    lo = (cols - hi.float()).to(torch.bfloat16)
    assert torch.equal(patches[0][:, : 3 * P * P], hi) and torch.equal(patches[1][:, : 3 * P * P], lo)
    assert not patches[:, :, 3 * P * P:].any()
    if n > 1:   # a batch equals single calls bit for bit
        for i in (0, n - 1):
            p1, _, _ = sc.preprocess(torch.from_numpy(fr[i: i + 1]))
            assert torch.equal(p1, patches[:, i * G * G: (i + 1) * G * G])


@pytest.mark.parametrize("S", [1, 5, 77, 197, 248, 257, 577])
@pytest.mark.parametrize("H", [1, 12, 16])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_f32_matches_fp64(hip_lib, parity, S, H, causal):
    from vist3a_amd import ops
    B, d = 3, H * 64
    g = torch.Generator().manual_seed(S * 100 + H)
    qkv = torch.randn(B * S, 3 * d, generator=g)
    qkv[:, :d] *= 1.5
    lens = torch.tensor([S, max(1, S // 2), max(1, S - 3)], dtype=torch.int32)
    dev = qkv.cuda()
    out = ops.attention_f32(dev[:, :d], dev[:, d: 2 * d], dev[:, 2 * d:], B=B, S=S, H=H, causal=causal, lens=lens.cuda(), out_f32=True)
    pair = ops.attention_f32(dev[:, :d], dev[:, d: 2 * d], dev[:, 2 * d:], B=B, S=S, H=H, causal=causal, lens=lens.cuda())
    again = ops.attention_f32(dev[:, :d], dev[:, d: 2 * d], dev[:, 2 * d:], B=B, S=S, H=H, causal=causal, lens=lens.cuda(), out_f32=True)
    assert torch.equal(out, again)
    hi = out.to(torch.bfloat16)
    assert torch.equal(pair[0], hi) and torch.equal(pair[1], (out - hi.float()).to(torch.bfloat16))
    q, k, v = (t.double().view(B, S, H, 64).transpose(1, 2) for t in qkv.split(d, 1))
    keep = (torch.arange(S)[None, :] < lens[:, None])[:, None, None, :].expand(B, 1, S, S).clone()
    if causal:
        keep &= torch.ones(S, S, dtype=torch.bool).tril()
    s = (q @ k.transpose(-1, -2)) * 0.125
    want = (s.masked_fill(~keep, float("-inf")).softmax(-1) @ v).transpose(1, 2).reshape(B * S, d)
    rows = torch.cat([torch.arange(S) + b * S for b in range(B)])
    if causal:   # rows past a sequence's valid length see no valid key beyond it: compare the rows a tower uses
        rows = torch.cat([torch.arange(int(lens[b])) + b * S for b in range(B)])
    err = rel(out[rows.cuda()], want[rows])
    parity(f"attention_f32 S={S} H={H} causal={causal}", rel_err=err)
    assert err <= GATES["attention"], err


def test_quick_gelu_epilogue_matches_fp64(hip_lib, parity):
    from vist3a_amd import lib as L, ops
    g = torch.Generator().manual_seed(5)
    M, K, N = 197, 768, 3072
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g) * 0.1
    cw = ops.ConvWeightSplit(w[:, :, None, None], b)
    y = ops.conv_split(ops.split_f32(x.cuda()).view(2, 1, 1, M, K), cw, act=L.ACT_QUICK_GELU)
    u = x.double() @ w.double().T + b.double()
    want = u * torch.sigmoid(1.702 * u)
    err = rel(ops.pair_value(y).view(M, N), want)
    parity("conv_split QUICK_GELU 197x768x3072", rel_err=err)
    assert err <= GATES["quick_gelu"], err
    plain = ops.conv_split(ops.split_f32(x.cuda()).view(2, 1, 1, M, K), cw, out_f32=True).view(M, N)
    e_plain = rel(plain, u)
    parity("conv_split 1x1 f32 out 197x768x3072", rel_err=e_plain)
    assert e_plain <= GATES["quick_gelu"]


@pytest.fixture(scope="module")
def golden():
    return load_file(str(ROOT / "tests" / "golden" / "clip_tiny.safetensors"))


def golden_model(golden, tag):
    from vist3a_amd.evaluation import clip as CL
    sd = {k[len(tag) + 3:]: v.float() if v.is_floating_point() else v for k, v in golden.items() if k.startswith(f"{tag}.w.")}
    hv, ht, eos, S, P = golden[f"{tag}.meta"].tolist()
    cfg = dict(text_config=dict(num_attention_heads=ht, eos_token_id=eos), vision_config=dict(num_attention_heads=hv))
    return sd, (hv, ht, eos, S, P), CL.ClipScorer(CL.ClipWeights.from_state_dict(cfg, sd, device="cuda"))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_tiny_goldens_end_to_end(hip_lib, golden, parity, tag):
    from vist3a_amd import ops
    sd, (hv, ht, eos, S, P), sc = golden_model(golden, tag)
    frames, ids, mask = golden[f"{tag}.frames"], golden[f"{tag}.input_ids"], golden[f"{tag}.attention_mask"]
    _, _, pix = sc.preprocess(frames, want_f32=True)
    assert torch.equal(pix.cpu(), golden[f"{tag}.pixel_values"])            # CLIPImageProcessorPil's own output, bit for bit
    ie, vh = sc.encode_images(frames, return_hidden=True)
    te, th = sc.encode_text(ids, mask, return_hidden=True)
    wi, wvh = CO.image_features(sd, golden[f"{tag}.pixel_values"], hv)
    wt, wth = CO.text_features(sd, ids, mask, ht, eos)
    e_img, e_txt = rel(ie, wi), rel(te, wt)
    e_vh = max(rel(a, b) for a, b in zip(vh, wvh))
    n = th[0].shape[1]
    e_th = max(rel(a[b, : min(n, int(mask[b].sum()))], w[b, : min(n, int(mask[b].sum()))]) for a, w in zip(th, wth) for b in range(ids.shape[0]))
    # against transformers' own fp32 output: the fp64 gate plus the golden's distance from fp64 (tests/test_clip_host.py)
    assert max(rel(ie, golden[f"{tag}.image_embeds"]), rel(te, golden[f"{tag}.text_embeds"])) <= GATES["golden_embed"] + 1.1e-6
    errs = []
    for b in range(ids.shape[0]):
        got = sc.score(frames, ids[b], mask[b])
        want = CO.clip_scores(wi, wt[b])
        errs.append((got.cpu() - want).abs().max().item())
        flipped = ops.clip_score(ie.contiguous(), (-te[b]).contiguous())[0]              # the clamp hides one sign: score the other too
        errs.append((flipped.cpu() - CO.clip_scores(wi, -wt[b])).abs().max().item())
        assert (got + flipped > 0).all()
        assert got.dtype == torch.float64
        assert abs(sc.prompt_score(frames, ids[b], mask[b]) - float(got.cpu().sum() / got.numel())) < 1e-12
    parity(f"clip tiny golden {tag}", image_rel=e_img, text_rel=e_txt, vision_hidden_rel=e_vh, text_hidden_rel=e_th, score_abs=max(errs))
    print(tag, dict(image=e_img, text=e_txt, vh=e_vh, th=e_th, score=max(errs)))
    assert max(e_img, e_txt) <= GATES["golden_embed"] and max(e_vh, e_th) <= GATES["golden_hidden"]
    assert max(errs) <= GATES["golden_score"]


DEEP = {
    "B16": dict(vision=dict(width=768, layers=12, inter=3072, patch=16, image=224), text=dict(width=512, layers=12, inter=2048, vocab=1000,
                                                                                         positions=77), proj=512, heads=(12, 8)),
    "L14": dict(vision=dict(width=1024, layers=24, inter=4096, patch=14, image=224), text=dict(width=768, layers=12, inter=3072, vocab=1000,
                                                                                          positions=248), proj=768, heads=(16, 12)),
}


def rendered_frames(n=8, W=448, H=448, U=4000, seed=21):
    """n views of a seeded Gaussian scene through the project's own rasteriser (ops.gs_render) -> uint8 [n,H,W,3] on the host"""
    import math
    from vist3a_amd import ops
    g = torch.Generator().manual_seed(seed)
    means = torch.randn(U, 3, generator=g) * torch.tensor([1.5, 1.5, 1.0]) + torch.tensor([0.0, 0.0, 4.0])
    A = torch.randn(U, 3, 3, generator=g) * 0.12
    cov = A @ A.transpose(1, 2) + 1e-4 * torch.eye(3)
    sh = (torch.randn(U, 3, 25, generator=g) * 0.3).contiguous()
    sh[:, :, 0] += torch.randn(U, 3, generator=g) * 1.2
    op = torch.rand(U, generator=g)
    views, Ks = [], []
    for i in range(n):
        yaw = 0.08 * i - 0.28
        c, s = math.cos(yaw), math.sin(yaw)
        v = torch.eye(4)
        v[:3, :3] = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        v[:3, 3] = torch.tensor([0.05 * i, 0.0, 0.1 * i])
        views.append(v)
        Ks.append(torch.tensor([[380.0 + 5 * i, 0, W / 2], [0, 400.0, H / 2], [0, 0, 1.0]]))
    view, K = torch.stack(views), torch.stack(Ks)
    campos = torch.stack([torch.linalg.inv(v.double())[:3, 3].float() for v in views]).contiguous()
    color, _, _ = ops.gs_render(means.cuda(), cov.cuda(), sh.cuda(), op.cuda(), view.cuda(), campos.cuda(), K.cuda(), W, H)
    u8 = (color.clamp(0, 1) * 255).round().to(torch.uint8).cpu()
    assert u8.shape == (n, H, W, 3) and u8.float().std() > 10          # a real picture, not a blank frame
    return u8


@pytest.mark.parametrize("name", ["B16", "L14"])
def test_production_models_per_block_and_end_to_end(hip_lib, parity, name):
    """ViT-B/16 (12 x 768, 197 tokens; text 12 x 512, 77 positions) and ViT-L/14 (24 x 1024, 257 tokens; text 12 x 768, 248 positions) at
    full depth with seeded full-fp32 weights, on 8 frames of 448^2 rendered by the rasteriser from a seeded scene: every block on the
    ORACLE's own input (per-block error), then embeddings and scores end to end against the fp64 oracle."""
    from vist3a_amd import ops
    from vist3a_amd.evaluation import clip as CL
    c = DEEP[name]
    sd = CO.seeded_state_dict(c["vision"], c["text"], c["proj"], seed=7)
    hv, ht = c["heads"]
    cfg = dict(text_config=dict(num_attention_heads=ht, eos_token_id=999), vision_config=dict(num_attention_heads=hv))
    sc = CL.ClipScorer(CL.ClipWeights.from_state_dict(cfg, sd, device="cuda"))
    frames = rendered_frames()
    L_txt = c["text"]["positions"]
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 999, (2, L_txt), generator=g)
    ids[0, L_txt - 1] = 999
    ids[1, L_txt // 3] = 999
    mask = (torch.arange(L_txt)[None] <= torch.tensor([[L_txt - 1], [L_txt // 3]])).long()
    pix = CO.preprocess(frames.numpy(), c["vision"]["image"])
    wi, wvh = CO.image_features(sd, pix, hv)
    wt, wth = CO.text_features(sd, ids, mask, ht, 999)
    N, S = wvh[0].shape[:2]
    blk = []
    for i, lw in enumerate(sc.w.vision.layers):
        y = sc.block(wvh[i].float().reshape(-1, wvh[i].shape[-1]).cuda().contiguous(), lw, sc.w.vision, N, S, False, None)
        blk.append(rel(y.view(N, S, -1), wvh[i + 1]))
    for i, lw in enumerate(sc.w.text.layers):
        y = sc.block(wth[i].float().reshape(-1, wth[i].shape[-1]).cuda().contiguous(), lw, sc.w.text, 2, L_txt, True, mask.sum(1).int().cuda())
        blk.append(rel(y.view(2, L_txt, -1)[0], wth[i + 1][0]))
    ie, te = sc.encode_images(frames), sc.encode_text(ids, mask)
    e_img, e_txt = rel(ie, wi), rel(te, wt)
    s_err = 0.0
    for b in range(2):
        for sign in (1.0, -1.0):
            got = ops.clip_score(ie.contiguous(), (sign * te[b]).contiguous())[0]
            s_err = max(s_err, (got.cpu() - CO.clip_scores(wi, sign * wt[b])).abs().max().item())
    assert torch.equal(sc.score(frames, ids[0], mask[0]), ops.clip_score(ie.contiguous(), te[0].contiguous())[0])
    parity(f"clip production model {name} full depth, 8 rasterised frames", block_rel_max=max(blk), image_rel=e_img, text_rel=e_txt,
           score_abs=s_err, fp32_spread=FP32_SPREAD)
    print(name, dict(block=max(blk), image=e_img, text=e_txt, score=s_err))
    assert max(blk) <= GATES["block"], blk
    assert max(e_img, e_txt) <= GATES["deep_embed"] and s_err <= GATES["deep_score"]


def test_exact_properties(hip_lib, golden):
    from vist3a_amd import ops
    sd, (hv, ht, eos, S, P), sc = golden_model(golden, "a")
    frames = torch.from_numpy(frames_of(80, 112, 8, seed=9))
    ids, mask = golden["a.input_ids"], golden["a.attention_mask"]
    s = sc.score(frames, ids[0], mask[0])
    assert torch.equal(s, sc.score(frames, ids[0], mask[0]))                                     # reruns
    perm = torch.tensor([3, 1, 7, 0, 2, 6, 5, 4])
    assert torch.equal(sc.score(frames[perm], ids[0], mask[0]), s[perm.cuda()])                  # frame order
    assert torch.equal(torch.cat([sc.score(frames[i: i + 1], ids[0], mask[0]) for i in range(8)]), s)   # batch size
    sc3 = type(sc)(sc.w, max_frames=3)
    assert torch.equal(sc3.score(frames, ids[0], mask[0]), s)
    te = sc.encode_text(ids, mask)
    assert torch.equal(te[0], sc.encode_text(ids[0], mask[0])[0]) and torch.equal(te[1], sc.encode_text(ids[1], mask[1])[0])
    # padding after EOS (tokens and mask) does not change the text embedding
    sdb, (_, _, eosb, _, _), scb = golden_model(golden, "b")
    idb, mkb = golden["b.input_ids"], golden["b.attention_mask"]
    base = scb.encode_text(idb[:1], mkb[:1])
    other = idb[:1].clone()
    other[0, 4:] = 33
    assert torch.equal(scb.encode_text(idb[:1, :4], mkb[:1, :4]), base) and torch.equal(scb.encode_text(other, None), base)
    # the clamp: a negative cosine scores exactly 0
    e = torch.randn(4, 32, generator=torch.Generator().manual_seed(0)).cuda()
    sco, mean = ops.clip_score(torch.cat([e, -e]), e[0].contiguous())
    assert sco[4].item() == 0.0 and abs(sco[0].item() - 100.0) < 1e-5 and (sco >= 0).all()
    assert torch.isnan(ops.clip_score(torch.zeros(1, 32).cuda(), e[0].contiguous())[0]).all()   # a zero embedding: NaN, as torchmetrics
    assert mean.item() == pytest.approx(sco.cpu().sum().item() / 8, abs=1e-12)
    # truncation at max_position_embeddings (16): a longer prompt scores as its explicit cut
    long_ids = torch.cat([ids[1], torch.tensor([4, 5, 6, 7, 8, 9, 10, 11, 12, 2])])
    assert long_ids.numel() > sc.w.max_positions
    assert torch.equal(sc.score(frames, long_ids), sc.score(frames, long_ids[: sc.w.max_positions]))
    with pytest.raises(ValueError):
        sc.encode_images(frames.float())
    with pytest.raises(RuntimeError, match="V3A_ERR_SHAPE"):
        ops.attention_f32(torch.zeros(4, 96).cuda(), torch.zeros(4, 96).cuda(), torch.zeros(4, 96).cuda(), B=1, S=4, H=1, head_dim=96)
    with pytest.raises(ValueError, match="device tensor"):
        ops.clip_score(torch.zeros(2, 8), torch.zeros(8))


def _tiny_clip_folder(folder: Path):
    """a local Hugging Face CLIPModel folder saved by the test: config.json, model.safetensors (seeded weights), preprocessor_config.json
    and a character-level CLIPTokenizerFast (byte alphabet, no merges; eos = pad = the last id, so pooling uses the first-EOS rule)"""
    import json
    from safetensors.torch import save_file
    from transformers import CLIPTokenizerFast
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, k = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + k)
            k += 1
    chars = [chr(c) for c in cs]
    vocab = {c: i for i, c in enumerate(chars)}
    vocab.update({c + "</w>": 256 + i for i, c in enumerate(chars)})
    vocab["<|startoftext|>"], vocab["<|endoftext|>"] = 512, 513
    folder.mkdir()
    CLIPTokenizerFast(vocab=vocab, merges=[]).save_pretrained(str(folder))
    vision, text = dict(width=64, layers=2, inter=128, patch=16, image=64), dict(width=64, layers=2, inter=128, vocab=514, positions=48)
    sd = CO.seeded_state_dict(vision, text, 32, seed=17)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(folder / "model.safetensors"))
    (folder / "config.json").write_text(json.dumps(dict(
        model_type="clip", projection_dim=32,
        text_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, vocab_size=514,
                         max_position_embeddings=48, eos_token_id=513, bos_token_id=512, pad_token_id=513, hidden_act="quick_gelu"),
        vision_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=64, patch_size=16,
                           hidden_act="quick_gelu"))))
    (folder / "preprocessor_config.json").write_text(json.dumps(dict(image_mean=[0.5, 0.45, 0.4], image_std=[0.25, 0.26, 0.27])))
    return sd


def test_cli_end_to_end(hip_lib, tmp_path):
    """evaluation/gen_eval/t3_scene_evaluation.py on the folder a weights-free `inference_t23d.py --synthetic_text` run writes, with a tiny
    seeded CLIP folder: the JSON equals ClipScorer called by hand on the same frames and token ids."""
    import json
    import subprocess
    from transformers import CLIPTokenizerFast
    import test_cli_gpu as TC
    from vist3a_amd.evaluation import clip as CL, gen_eval as GE
    assets = TC._write_assets(tmp_path)
    out = tmp_path / "results"
    r = TC._cli(assets, out)
    assert r.returncode == 0, r.stderr[-3000:]
    (out / "incomplete").mkdir()
    (out / "incomplete" / "prompt.txt").write_text("no video here\n")
    model = tmp_path / "clip-tiny"
    _tiny_clip_folder(model)
    res = tmp_path / "eval.json"
    cmd = [sys.executable, str(ROOT / "evaluation" / "gen_eval" / "t3_scene_evaluation.py"), "--folder_path", str(out),
           "--eval_save_path", str(res), "--clip_model", str(model)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Skipping incomplete: missing gs.mp4 or prompt.txt" in r.stdout
    got = json.loads(res.read_text())
    assert set(got) == {"all_average", "eval_results"} and set(got["all_average"]) == {"clip_score"}
    sc = CL.ClipScorer(CL.ClipWeights.from_pretrained(model))
    assert sc.w.mean == (0.5, 0.45, 0.4) and sc.w.eos_token_id == 513 and sc.w.max_positions == 48
    tok = CLIPTokenizerFast.from_pretrained(str(model), local_files_only=True)
    want = []
    for prompt, video in GE.get_file_list_with_pair(str(out)).items():
        frames = torch.from_numpy(GE.sample_video_frames(video))
        assert frames.shape[0] == 8 and frames.shape[1:] == (448, 448, 3)
        enc = tok([prompt], padding=True, return_tensors="pt")
        s = sc.score(frames, enc["input_ids"], enc["attention_mask"])
        want.append({"prompt": prompt, "clip_score": float(s.cpu().sum().item() / 8)})
        assert abs(want[-1]["clip_score"] - sc.prompt_score(frames, enc["input_ids"], enc["attention_mask"])) < 1e-12
    assert [w["prompt"] for w in want] == sorted(assets.prompts.read_text().splitlines())
    assert len(got["eval_results"]) == 2
    for g_row, w_row in zip(got["eval_results"], want):
        assert set(g_row) == {"prompt", "clip_score"} and g_row["prompt"] == w_row["prompt"]
        assert abs(g_row["clip_score"] - w_row["clip_score"]) < 1e-12, (g_row, w_row)
    assert abs(got["all_average"]["clip_score"] - sum(w["clip_score"] for w in want) / 2) < 1e-12
    # a prompt longer than the 48 positions scores as its explicit cut, through the tokenizer path as well
    long = tok(["x" * 80], return_tensors="pt")
    assert long["input_ids"].shape[1] > 48
