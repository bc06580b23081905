"""Timing of the CLIP score (vist3a_amd.evaluation.clip) on one MI355X: ms per 8-frame prompt at 448^2 input for ViT-B/16 and ViT-L/14
shapes with seeded weights, split into resize / towers (of which attention) / head, and the executed TFLOP/s of the split GEMMs (three
bf16 products per fp32-equivalent product) against the bf16 matrix roof.

    python tools/clip_time.py [reps]        -> one JSON line per model"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import clip_oracle as CO  # noqa: E402
from vist3a_amd import ops  # noqa: E402
from vist3a_amd.evaluation import clip as CL  # noqa: E402

MODELS = {
    "ViT-B/16": dict(vision=dict(width=768, layers=12, inter=3072, patch=16, image=224), text=dict(width=512, layers=12, inter=2048, vocab=49408,
                                                                                              positions=77), proj=512, heads=(12, 8)),
    "ViT-L/14": dict(vision=dict(width=1024, layers=24, inter=4096, patch=14, image=224), text=dict(width=768, layers=12, inter=3072, vocab=49408,
                                                                                               positions=248), proj=768, heads=(16, 12)),
}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (8, 448, 448, 3), dtype=np.uint8)).cuda()
    for name, c in MODELS.items():
        sd = CO.seeded_state_dict(c["vision"], c["text"], c["proj"], seed=7)
        cfg = dict(text_config=dict(num_attention_heads=c["heads"][1], eos_token_id=49407), vision_config=dict(num_attention_heads=c["heads"][0]))
        sc = CL.ClipScorer(CL.ClipWeights.from_state_dict(cfg, sd, device="cuda"))
        ids = torch.randint(0, 49000, (1, 24))
        ids[0, -1] = 49407
        patches, _, _ = sc.preprocess(frames)
        img, txt = sc.encode_images(frames).contiguous(), sc.encode_text(ids).contiguous()
        d, H, S = c["vision"]["width"], c["heads"][0], (c["vision"]["image"] // c["vision"]["patch"]) ** 2 + 1
        qkv = torch.randn(8 * S, 3 * d, device="cuda")
        meter = ops.FlopMeter()
        ops.set_flop_meter(meter)
        sc.encode_patches(patches, 8)
        ops.set_flop_meter(None)
        t = dict(resize=timed(lambda: sc.preprocess(frames), reps), vision=timed(lambda: sc.encode_patches(patches, 8), reps),
                 text=timed(lambda: sc.encode_text(ids), reps),
                 attention_one_layer=timed(lambda: ops.attention_f32(qkv[:, :d], qkv[:, d: 2 * d], qkv[:, 2 * d:], B=8, S=S, H=H), reps),
                 head=timed(lambda: ops.clip_score(img, txt[0].contiguous()), reps), total=timed(lambda: sc.score(frames, ids), reps))
        att = t["attention_one_layer"] * c["vision"]["layers"]
        gemm_ms = t["vision"] - att
        x = torch.randn(8 * S, d, device="cuda")
        pe = torch.randn(8 * (S - 1), d, device="cuda")
        t["token_assembly"] = timed(lambda: ops.clip_rows(pe, cls=sc.w.cls, pos=sc.w.vision_pos, S=S), reps)
        t["layernorm_pair"] = timed(lambda: ops.layernorm_pair(x, weight=sc.w.pre_ln[0], bias=sc.w.pre_ln[1]), reps)
        tab = sc.tables(448, 448)
        # bytes every streaming pass has to move at least once (reads + writes); GB/s = bytes / time, against HBM's 8 TB/s peak
        bytes_ = dict(resize=frames.numel() + 2 * 8 * tab["rows"] * 224 * 3 + patches.numel() * 2,
                      token_assembly=(pe.numel() + x.numel()) * 4, layernorm_pair=x.numel() * 4 + x.numel() * 4)
        att_flops = 4.0 * 8 * H * S * S * 64
        print(json.dumps(dict(model=name, ms_per_8_frame_prompt=t, vision_attention_ms=att, vision_attention_share=att / t["vision"],
                              attention_fp32_tflops=att_flops / (t["attention_one_layer"] * 1e-3) / 1e12,
                              vision_split_gemm_executed_tflops=3 * meter.total / (gemm_ms * 1e-3) / 1e12,
                              vision_split_gemm_useful_tflops=meter.total / (gemm_ms * 1e-3) / 1e12,
                              streaming_gb_per_s={k: v / (t[k] * 1e-3) / 1e9 for k, v in bytes_.items()},
                              device=torch.cuda.get_device_name(0))), flush=True)

if __name__ == "__main__":
    main()
