#!/usr/bin/env python3
"""Digests of the training decoder tape on seeded inputs, to compare two commits: per case the sha256 of every level's
logits, of every gradient in name order and of dL/d(pcd_features), and the sha256 of the call trace -- the ordered list of
(symbol, every argument that is not a pointer) of all library calls made by forward + backward.  Cases: FLASH on / off x
dropout 0 / 0.1 (fixed seed) x a one-sample tape of 3000 voxels / a batched tape of 3000 + 700 voxels (the small sample takes
the materialised path even with FLASH on), 12 clicks on 3 objects per sample.  Only DecoderTape's constructor, backward()
and release() and setattr on the loaded library's symbols are used, so the same file runs on either commit:
  python tools/tape_digest.py [--json digests.json] [--tensors values.pt]"""
import argparse, hashlib, json, os, sys
import torch
import lib_trace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agile3d_amd import build_model, default_args
from agile3d_amd import train_decoder as TD
from agile3d_amd.synthetic import make_clicks, make_scene

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="", help="write {case: {name: sha256}} here")
ap.add_argument("--tensors", default="", help="torch.save {case: {name: tensor}} here (to compare runs that differ in bits)")
args = ap.parse_args()


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


trace = lib_trace.install()

torch.manual_seed(0)
model = build_model(default_args(dropout=0.1)).cuda().train()
samples = []
for n, seed in ((3000, 1), (700, 2)):
    sc = make_scene(n, seed=seed)
    g = torch.Generator().manual_seed(seed)
    rows = len(sc["coords"])
    ci, ct = make_clicks(sc["labels"], n_objects=3, clicks_per_object=4, n_bg_clicks=0, seed=seed)
    samples.append((torch.randn(rows, 128, generator=g).cuda() * 0.3, torch.randn(rows, 128, generator=g).cuda() * 0.3, ci, ct,
                    [torch.randn(rows, 4, generator=g).cuda() / 8 for _ in range(model.num_decoders)]))

digests, tensors = {}, {}
for flash in (True, False):
    for p in (0.0, 0.1):
        for batched in (False, True):
            case = f"flash={int(flash)} dropout={p} {'batch 3000+700' if batched else 'one 3000'}"
            use = samples if batched else samples[:1]
            TD.FLASH = flash
            del trace[:]
            try:
                if batched:
                    tape = TD.DecoderTape(model, *[[s[i] for s in use] for i in range(4)], dropout=p, seed=0x5eed_0123)
                    d_logits = [[s[4][l] for s in use] for l in range(model.num_decoders)]
                    logits = {f"logits[{l}][{b}]": t for l, lvl in enumerate(tape.logits) for b, t in enumerate(lvl)}
                else:
                    tape = TD.DecoderTape(model, *use[0][:4], dropout=p, seed=0x5eed_0123)
                    d_logits = use[0][4]
                    logits = {f"logits[{l}]": t for l, t in enumerate(tape.logits)}
                grads, d_pcd = tape.backward(d_logits)
            finally:
                TD.FLASH = True
            torch.cuda.synchronize()
            vals = dict(logits, d_pcd=d_pcd, **{f"grad {k}": grads[k] for k in sorted(grads)})
            digests[case] = {k: sha(v) for k, v in vals.items()}
            digests[case]["values"] = hashlib.sha256("".join(digests[case][k] for k in vals).encode()).hexdigest()
            digests[case]["trace"] = lib_trace.digest(trace)
            digests[case]["calls"] = len(trace)
            if args.tensors:
                tensors[case] = {k: v.detach().cpu().clone() for k, v in vals.items()}
            tape.release()
            print(f"{case} | calls {len(trace)} | trace {digests[case]['trace'][:16]} | values {digests[case]['values'][:16]}", flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(digests, f, indent=1)
if args.tensors:
    torch.save(tensors, args.tensors)
