"""Host side of the CLIP score (vist3a_amd.evaluation.clip / gen_eval, evaluation/gen_eval/t3_scene_evaluation.py): no GPU.

Measured here (printed by the tests): the fp64 oracle (tests/clip_oracle.py) against the transformers golden - image / text embeddings
3.3e-7 / 3.2e-7 relative, hidden states up to 5.4e-7 (the golden is fp32 torch); the fp32 oracle against the fp64 oracle - embeddings 3.8e-7,
hidden states 5.4e-7: the spread the GPU path is judged against (tests/test_clip_gpu.py)."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image
from safetensors.torch import load_file

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402
from vist3a_amd.evaluation import clip as CL  # noqa: E402
from vist3a_amd.evaluation import gen_eval as GE  # noqa: E402

SHAPES = [((448, 448), 224), ((448, 448), 378), ((512, 512), 224), ((360, 640), 224), ((301, 517), 224), ((96, 70), 224), ((224, 224), 224)]
# twice the largest figure measured (see the module docstring): the golden is fp32 torch, so about 1e-6 relative is what fp64 can reach
GOLDEN_GATE = 1.1e-6   # measured 5.42e-7
SPREAD_GATE = 1.1e-6   # measured 5.40e-7


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def images(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([127 + 120 * np.sin(0.05 * (c + 1) * x + 0.03 * y + c) for c in range(3)], -1).round().astype(np.uint8)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8), smooth]


@pytest.mark.parametrize("hw,size", SHAPES)
def test_coefficient_tables_reproduce_pillow_bicubic(hw, size):
    H, W = hw
    oh, ow, top, left = CL.resize_geometry(H, W, size)
    xb, xk = CL.pillow_bicubic_coeffs(W, ow)
    yb, yk = CL.pillow_bicubic_coeffs(H, oh)
    t = CL.resize_tables_host(H, W, size)
    for img in images(H, W):
        want = np.asarray(Image.fromarray(img).resize((ow, oh), resample=Image.BICUBIC))
        assert np.array_equal(CL.resample_numpy(img, xb, xk, yb, yk), want)
        # the crop's tables alone, on the rows the vertical taps read
        sub = img[t["row0"]: t["row0"] + t["rows"]]
        ybs = t["y_bounds"].copy()
        ybs[:, 0] -= t["row0"]
        got = CL.resample_numpy(sub, t["x_bounds"], t["x_coeffs"], ybs, t["y_coeffs"])
        assert np.array_equal(got, want[top: top + size, left: left + size])


@pytest.mark.parametrize("hw", [(360, 640), (640, 360), (448, 448), (301, 517), (96, 70)])
def test_geometry_matches_the_processor(hw):
    from transformers.image_transforms import center_crop, get_resize_output_image_size
    H, W = hw
    img = np.zeros((H, W, 3), np.uint8)
    oh, ow = get_resize_output_image_size(img, size=224, default_to_square=False, input_data_format="channels_last")
    goh, gow, top, left = CL.resize_geometry(H, W, 224)
    assert (goh, gow) == (oh, ow)
    marks = np.arange(oh * ow, dtype=np.float32).reshape(oh, ow, 1).repeat(3, 2)
    crop = center_crop(marks, (224, 224), input_data_format="channels_last")
    assert crop[0, 0, 0] == top * ow + left and crop.shape[:2] == (224, 224)


def test_normalise_table_matches_transformers():
    from transformers.image_transforms import normalize, rescale
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    want = normalize(rescale(u, 1 / 255, input_data_format="channels_last"), CL.CLIP_MEAN, CL.CLIP_STD, input_data_format="channels_last")
    assert want.dtype == np.float32
    assert np.array_equal(CL.normalize_lut().T.reshape(16, 16, 3), want)


@pytest.fixture(scope="module")
def golden():
    return load_file(str(ROOT / "tests" / "golden" / "clip_tiny.safetensors"))


def cfg_of(golden, tag):
    sd = {k[len(tag) + 3:]: v.float() if v.is_floating_point() else v for k, v in golden.items() if k.startswith(f"{tag}.w.")}
    hv, ht, eos, S, P = golden[f"{tag}.meta"].tolist()
    return sd, hv, ht, eos, S, P


@pytest.mark.parametrize("tag", ["a", "b"])
def test_oracle_reproduces_the_golden(golden, tag):
    sd, hv, ht, eos, S, P = cfg_of(golden, tag)
    pv = golden[f"{tag}.pixel_values"]
    assert np.array_equal(CO.preprocess(golden[f"{tag}.frames"].numpy(), S), pv.numpy())   # the Pillow path, bit for bit
    ids, mask = golden[f"{tag}.input_ids"], golden[f"{tag}.attention_mask"]
    ie, vh = CO.image_features(sd, pv, hv)
    te, th = CO.text_features(sd, ids, mask, ht, eos)
    errs = {"image": rel(ie, golden[f"{tag}.image_embeds"]), "text": rel(te, golden[f"{tag}.text_embeds"])}
    for i, h in enumerate(vh):
        errs[f"vision_hidden.{i}"] = rel(h, golden[f"{tag}.vision_hidden.{i}"])
    # text rows after a prompt's padding start are not comparable (transformers masks padded keys for them too): compare valid rows
    for i, h in enumerate(th):
        g = golden[f"{tag}.text_hidden.{i}"]
        for b in range(ids.shape[0]):
            n = int(mask[b].sum())
            errs[f"text_hidden.{i}.{b}"] = rel(h[b, :n], g[b, :n])
    print(tag, "fp64 oracle vs golden", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= GOLDEN_GATE, errs
    # logits_per_image = exp(logit_scale) * cosine
    cos = torch.stack([CO.clip_scores(ie, t) for t in te], 1) / 100
    lp = golden[f"{tag}.logits_per_image"].double() / sd["logit_scale"].double().exp()
    assert ((cos - lp.clamp(min=0)).abs().max() < 1e-6)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fp32_oracle_spread(golden, tag):
    """fp32 torch against fp64 torch: the spread a correct fp32 implementation shows on these models"""
    sd, hv, ht, eos, S, P = cfg_of(golden, tag)
    pv, ids, mask = golden[f"{tag}.pixel_values"], golden[f"{tag}.input_ids"], golden[f"{tag}.attention_mask"]
    i64, vh64 = CO.image_features(sd, pv, hv)
    i32, vh32 = CO.image_features(sd, pv, hv, dtype=torch.float32)
    t64, _ = CO.text_features(sd, ids, mask, ht, eos)
    t32, _ = CO.text_features(sd, ids, mask, ht, eos, dtype=torch.float32)
    spread = dict(image=rel(i32, i64), text=rel(t32, t64), hidden=max(rel(a, b) for a, b in zip(vh32, vh64)))
    print(tag, "fp32 oracle vs fp64 oracle", {k: f"{v:.2e}" for k, v in spread.items()})
    assert max(spread.values()) <= SPREAD_GATE, spread


def test_eos_pooling_rules_and_padding(golden):
    ids = torch.tensor([[5, 9, 2, 41, 58, 3, 1], [7, 59, 9, 59, 11, 12, 13]])
    assert CL.eos_positions(ids, 2).tolist() == [4, 1]        # argmax(input_ids): the largest id, first occurrence
    assert CL.eos_positions(ids, 59).tolist() == [0, 1]       # first position of eos_token_id; absent -> 0
    sd, hv, ht, eos, S, P = cfg_of(golden, "b")
    ids, mask = golden["b.input_ids"], golden["b.attention_mask"]
    base, _ = CO.text_features(sd, ids, mask, ht, eos)
    cut, _ = CO.text_features(sd, ids[:1, :4], mask[:1, :4], ht, eos)          # the first prompt without its padding
    assert torch.equal(cut[0], base[0]) or rel(cut[0], base[0]) < 1e-14
    other = ids.clone()
    other[0, 4:] = 33                                                           # different padding tokens after EOS
    moved, _ = CO.text_features(sd, other, None, ht, eos)
    assert rel(moved[0], base[0]) < 1e-14


def jpeg(arr, q=90):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="JPEG", quality=q)
    return b.getvalue()


@pytest.mark.parametrize("n", [8, 20, 132])
def test_avi_reader_and_sampling(tmp_path, n):
    from vist3a_amd.misc.image_io import _write_mjpeg_avi
    rng = np.random.default_rng(n)
    H, W = 24, 40
    blobs = [jpeg(np.clip(rng.normal(128, 40, (H, W, 3)) + i, 0, 255).astype(np.uint8)) for i in range(n)]
    p = tmp_path / "gs.avi"
    _write_mjpeg_avi(p, blobs, W, H, 20)
    assert GE.mjpeg_avi_chunks(p) == blobs
    frames = GE.read_mjpeg_avi(p)
    assert frames.shape == (n, H, W, 3) and frames.dtype == np.uint8
    for i in (0, n // 2, n - 1):
        assert np.array_equal(frames[i], np.asarray(Image.open(io.BytesIO(blobs[i])).convert("RGB")))
    idx = GE.sample_indices(n)
    assert idx == [int(i * n / 8) for i in range(8)] and len(idx) == 8
    assert np.array_equal(GE.sample_video_frames(p), frames[idx])


def test_mp4_without_opencv_names_the_file(tmp_path, monkeypatch):
    from vist3a_amd.misc.image_io import _write_mjpeg_avi
    monkeypatch.setitem(sys.modules, "cv2", None)          # `import cv2` raises ImportError, whether or not OpenCV is installed
    seq = tmp_path / "res" / "s0"
    seq.mkdir(parents=True)
    (seq / "prompt.txt").write_text("a prompt\n")
    p = seq / "gs.mp4"
    p.write_bytes(b"\0" * 32)
    with pytest.raises(RuntimeError, match="gs.mp4"):
        GE.sample_video_frames(p)
    assert GE.get_file_list_with_pair(str(tmp_path / "res")) == {"a prompt": str(p)}
    # a readable gs.avi beside it is preferred when OpenCV is missing
    _write_mjpeg_avi(seq / "gs.avi", [jpeg(np.zeros((16, 16, 3), np.uint8))] * 8, 16, 16, 20)
    assert GE.get_file_list_with_pair(str(tmp_path / "res")) == {"a prompt": str(seq / "gs.avi")}


def test_cli_on_a_temporary_folder(tmp_path, capsys):
    from vist3a_amd.misc.image_io import _write_mjpeg_avi
    sys.path.insert(0, str(ROOT / "evaluation" / "gen_eval"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("t3_scene_evaluation", ROOT / "evaluation" / "gen_eval" / "t3_scene_evaluation.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    res = tmp_path / "results"
    for k, (name, prompt) in enumerate([("s0", "a red chair\nsecond line"), ("s1", "a blue sofa")]):
        (res / name).mkdir(parents=True)
        (res / name / "prompt.txt").write_text(prompt + "\n")
        _write_mjpeg_avi(res / name / "gs.avi", [jpeg(np.full((16, 16, 3), 10 * i + k, np.uint8)) for i in range(10)], 16, 16, 20)
    (res / "s2").mkdir()
    (res / "s2" / "prompt.txt").write_text("no video\n")
    (res / "s3").mkdir()
    _write_mjpeg_avi(res / "s3" / "gs.avi", [jpeg(np.zeros((16, 16, 3), np.uint8))], 16, 16, 20)
    (res / "stray.txt").write_text("x")
    model = tmp_path / "clip"
    model.mkdir()
    (model / "config.json").write_text("{}")
    seen = []

    def stub(model_dir):
        def fn(frames, prompt):
            seen.append((prompt, frames.shape))
            return float(len(prompt))
        return fn
    out_path = tmp_path / "eval.json"
    cli.main(cli.parse_args(["--folder_path", str(res), "--eval_save_path", str(out_path), "--clip_model", str(model)]), make_scorer=stub)
    text = capsys.readouterr().out
    assert "Skipping s2: missing gs.mp4 or prompt.txt" in text and "Skipping s3: missing gs.mp4 or prompt.txt" in text
    out = json.loads(out_path.read_text())
    assert set(out) == {"all_average", "eval_results"}
    assert set(out["all_average"]) == {"clip_score"}
    assert out["eval_results"] == [{"prompt": "a red chair", "clip_score": 11.0}, {"prompt": "a blue sofa", "clip_score": 11.0}]
    assert out["all_average"]["clip_score"] == 11.0
    assert seen == [("a red chair", (8, 16, 16, 3)), ("a blue sofa", (8, 16, 16, 3))]
    with pytest.raises(SystemExit, match="not a local Hugging Face model folder"):
        cli.main(cli.parse_args(["--folder_path", str(res), "--clip_model", str(tmp_path / "missing")]), make_scorer=stub)
    with pytest.raises(SystemExit, match="nothing to compute"):
        cli.main(cli.parse_args(["--folder_path", str(res)]), make_scorer=stub)


def test_loader_consumes_every_key(golden, monkeypatch):
    """every key of a CLIPModel.state_dict() is packed or named in UNUSED_KEYS (packing runs on the host)"""
    from transformers import CLIPConfig, CLIPModel
    sd, hv, ht, eos, S, P = cfg_of(golden, "b")
    cfg = CLIPConfig(text_config=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1, vocab_size=60,
                                      max_position_embeddings=12, eos_token_id=59),
                     vision_config=dict(hidden_size=64, intermediate_size=64, num_hidden_layers=2, num_attention_heads=1, image_size=56,
                                        patch_size=14), projection_dim=32)
    full = CLIPModel(cfg).state_dict()
    assert set(sd) <= set(full) | set(CL.UNUSED_KEYS)
    config = dict(text_config=dict(num_attention_heads=1, eos_token_id=59), vision_config=dict(num_attention_heads=1))
    w = CL.ClipWeights.from_state_dict(config, dict(full), device="cpu")
    assert set(w.unused) <= set(CL.UNUSED_KEYS)
    assert (w.image_size, w.patch, w.grid, w.max_positions, w.eos_token_id, w.proj_dim) == (56, 14, 4, 12, 59, 32)
    assert w.patch_w.CinP == 592 and len(w.vision.layers) == 2 and len(w.text.layers) == 1
    bad = dict(full)
    bad["vision_model.extra.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match="vision_model.extra.weight"):
        CL.ClipWeights.from_state_dict(config, bad, device="cpu")
    with pytest.raises(ValueError, match="head size"):
        CL.ClipWeights.from_state_dict(dict(config, vision_config=dict(num_attention_heads=2)), dict(full), device="cpu")
