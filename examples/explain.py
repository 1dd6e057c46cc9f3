#!/usr/bin/env python
"""Which time columns make the model say a label: gradient-weighted attention rollout (MAEST.attention_relevance) for the top
predictions of a clip (random noise unless --wav-npy points at a float32 mono 16 kHz array), and which heads of which blocks carry the
evidence for the first of them (MAEST.attention_heads).  --faithfulness adds the perturbation test (MAEST.perturbation_curve): for rollout,
relevance and a random ranking, the area under the label's probability while the highest / the lowest scored patches are removed.

    python examples/explain.py --seconds 30 [--label "Rock---Shoegaze"] [--checkpoint model.ckpt] [--faithfulness]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maest import get_maest  # noqa: E402  (alias package of maest_amd, as in the reference)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="discogs-maest-30s-pw-129e")
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--wav-npy", default=None, help="float32 mono 16 kHz samples saved with numpy.save")
    ap.add_argument("--checkpoint", default=None, help="Lightning .ckpt with net_swa.* / net.* weights")
    ap.add_argument("--label", default=None, help="a label of the model's list; default: the top three predictions")
    ap.add_argument("--precision", default="auto", choices=["auto", "fp32", "bf16", "bf16x3", "fp16"])
    ap.add_argument("--faithfulness", action="store_true", help="perturbation curves of rollout, relevance and a random ranking")
    args = ap.parse_args()

    model = get_maest(args.arch, pretrained=False, checkpoint=args.checkpoint, precision=args.precision).cuda().eval()
    if args.wav_npy:
        audio = torch.from_numpy(np.load(args.wav_npy).astype(np.float32)).cuda()
    else:
        rng = np.random.Generator(np.random.PCG64(0))
        audio = torch.from_numpy((rng.standard_normal(int(args.seconds * 16000)) * 0.1).astype(np.float32)).cuda()
    activations, labels = model.predict_labels(audio)
    wanted = [labels.index(args.label)] if args.label else np.argsort(activations)[::-1][:3].tolist()
    scale = 1024.0 if args.precision == "fp16" else 1.0     # half gradients underflow without it; exact in every other mode
    for c in wanted:
        r = model.attention_relevance(audio, int(c), grad_scale=scale)
        per_t = torch.nan_to_num(r.to_grid(row=0)[0]).sum(0)             # cls row of chunk 0, summed over frequency: [T']
        best = torch.topk(per_t, 5).indices.tolist()
        print(f"{activations[c]:.3f}  {labels[c]}: top time columns of chunk 0 (of {r.grid[1]}; 0.16 s apart): "
              + ", ".join(f"t={t} ({per_t[t].item():.2e})" for t in best))
    # which heads carry the evidence for the first of them: the same walk, every block's step kept per head (MAEST.attention_heads)
    c = wanted[0]
    h = model.attention_heads(audio, int(c), grad_scale=scale)
    scores = h.head_scores(row=0)[0]                                     # cls row of chunk 0: [blocks, 12]
    top = torch.topk(scores.flatten(), 5)
    print(f"{labels[c]}: heads that pass on the most relevance in chunk 0: "
          + ", ".join(f"block {i // 12} head {i % 12} ({v:.2e})" for v, i in zip(top.values.tolist(), top.indices.tolist())))
    if args.faithfulness:
        # a faithful map: the probability falls fast when its highest scores leave first (small positive area) and slowly when its
        # lowest do (large negative area); the random ranking is the baseline of both
        maps = {"rollout": model.attention_rollout(audio), "relevance": model.attention_relevance(audio, int(c), grad_scale=scale),
                "random": "random"}
        print(f"{labels[c]}: area under the probability per chunk, patches removed in 10 % steps (positive / negative order)")
        for name, m in maps.items():
            pos = model.perturbation_curve(audio, m, int(c), order="positive")
            neg = model.perturbation_curve(audio, m, int(c), order="negative")
            print(f"  {name:>9}: " + "  ".join(f"{p:.3f} / {n:.3f}" for p, n in zip(pos.auc.tolist(), neg.auc.tolist())))


if __name__ == "__main__":
    main()
