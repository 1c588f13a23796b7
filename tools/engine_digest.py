#!/usr/bin/env python3
"""Digests of the engine's host code (agile3d_amd/engine.py: what ``Agile3d.forward_backbone`` / ``forward_mask`` go through)
on a seeded model and small seeded scenes, to compare two commits: per case the sha256 of the outputs, of the call trace --
the ordered list of (symbol, every argument that is not a pointer) of the library calls made -- with its length, and of the
backbone op program (every non-pointer ``a3d_op`` field, which pointers are set, ``pool.descs``).  Cases:
  eval      forward_backbone + forward_mask on one 3000-voxel scene and on a batch of 3000 + 700 voxels, 3 objects x 4 clicks,
            each without and with background clicks
  cache     three consecutive forward_mask calls on one backbone output (scene-cache states 0, 1, 2)
  inputs    decoder_inputs and decoder_inputs_batch fed the same features, and forward_mask on each
  train     training-mode forward_backbone + forward_mask + backward() through autograd.py, ``.grad`` in name order
  unfused   BackboneProgram(fuse_proj=False) and one run of it
Only public names of the model and the engine's documented attributes (``program.ops_arr`` / ``pool.descs`` /
``fused_projections`` / ``run``, ``decoder_inputs``, ``decoder_inputs_batch``, ``_a3d``) are used, so the same file runs
on either commit:
  python tools/engine_digest.py [--json digests.json]"""
import argparse, ctypes, hashlib, json, os, sys
import numpy as np
import torch
import lib_trace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from agile3d_amd import SparseTensor, build_model, default_args, randomize_bn_stats
from agile3d_amd import lib as L
from agile3d_amd.engine import BackboneProgram, Scene
from agile3d_amd.synthetic import make_clicks, make_scene

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="", help="write {case: {name: sha256 or call count}} here")
args = ap.parse_args()
trace = lib_trace.install()
digests = {}


def sha(values):
    h = hashlib.sha256()
    for v in values:
        h.update(b"none" if v is None else v.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def program_digest(prog):
    ops = [tuple(bool(getattr(o, f)) if t is ctypes.c_void_p else getattr(o, f) for f, t in L.Op._fields_) for o in prog.ops_arr]
    return hashlib.sha256(repr((ops, list(prog.pool.descs), prog.fused_projections)).encode()).hexdigest()


def record(case, values, prog=None):
    torch.cuda.synchronize()
    d = digests[case] = {"outputs": sha(values), "trace": lib_trace.digest(trace), "calls": len(trace)}
    line = f"{case} | outputs {d['outputs'][:16]} | trace {d['trace'][:16]} [{d['calls']} calls]"
    if prog is not None:
        d["program"] = program_digest(prog)
        line += f" | program {d['program'][:16]} [{prog.n_ops} ops, {len(prog.pool.descs)} buffers]"
    print(line, flush=True)
    del trace[:]


def masks(out):
    return [m for a in out.get("aux_outputs", []) for m in a["pred_masks"]] + list(out["pred_masks"])


torch.manual_seed(0)
model = randomize_bn_stats(build_model(default_args())).eval().cuda()
state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
dev = torch.device("cuda")
scenes = [make_scene(3000, seed=1), make_scene(700, seed=2, batch_index=1)]
clicks = {bg: [make_clicks(sc["labels"], n_objects=3, clicks_per_object=4, n_bg_clicks=bg, seed=i + 1) for i, sc in enumerate(scenes)]
          for bg in (0, 2)}


def inputs(ns):
    cat = lambda k: torch.from_numpy(np.concatenate([sc[k] for sc in scenes[:ns]]))
    return SparseTensor(features=cat("feats"), coordinates=cat("coords"), device=dev), cat("raw_xyz").to(dev)


# ---- eval: one scene / a batch, without / with background clicks
for ns, name in ((1, "one 3000"), (2, "batch 3000+700")):
    for bg in (0, 2):
        x, raw = inputs(ns)
        del trace[:]
        r = model.forward_backbone(x, raw_coordinates=raw)
        out = model.forward_mask(*r, click_idx=[c[0] for c in clicks[bg][:ns]], click_time_idx=[c[1] for c in clicks[bg][:ns]])
        record(f"eval {name}, {bg} background clicks", [r[0].F, r[2].F] + [a.F for a in r[1]] + list(r[3][4][0]) + masks(out),
               model._get_engine().program)

# ---- cache: three forward_mask calls on one backbone output
x, raw = inputs(2)
r = model.forward_backbone(x, raw_coordinates=raw)
ci, ct = [c[0] for c in clicks[2]], [c[1] for c in clicks[2]]
del trace[:]
for call in range(3):
    out = model.forward_mask(*r, click_idx=ci, click_time_idx=ct)
    st = r[0]._a3d
    record(f"cache forward_mask call {call + 1} (mask_calls {st.mask_calls}, cache {'filled' if st.kv0 is not None else 'empty'})", masks(out))

# ---- inputs: decoder_inputs / decoder_inputs_batch on the same features
eng = model._get_engine()
g = torch.Generator().manual_seed(5)
n0 = len(scenes[0]["coords"])
feats = torch.randn(n0, 128, generator=g) * 0.3
raw0 = torch.from_numpy(scenes[0]["raw_xyz"])
del trace[:]
for name, r in (("decoder_inputs", eng.decoder_inputs(feats, raw0)),
                ("decoder_inputs_batch", eng.decoder_inputs_batch(feats, raw0, [(0, n0)]))):
    out = model.forward_mask(*r, click_idx=ci[:1], click_time_idx=ct[:1])
    record(f"inputs {name} + forward_mask", [r[0].F, r[0].C, r[2].F] + list(r[3][4][0]) + [m for m in r[0]._a3d.minmax] + masks(out))
n1 = len(scenes[1]["coords"])
feats2 = torch.cat([feats, torch.randn(n1, 128, generator=g) * 0.3])
r = eng.decoder_inputs_batch(feats2, inputs(2)[1], [(0, n0), (n0, n0 + n1)])
out = model.forward_mask(*r, click_idx=ci, click_time_idx=ct)
record("inputs decoder_inputs_batch of two samples + forward_mask", [r[0].F, r[0].C, r[2].F] + list(r[3][4][0]) + masks(out))

# ---- train: both training-mode forwards and backward() through autograd.py
model.train()
model.zero_grad()
x, raw = inputs(1)
del trace[:]
r = model.forward_backbone(x, raw_coordinates=raw)
out = model.forward_mask(*r, click_idx=ci[:1], click_time_idx=ct[:1])
logits = masks(out)
loss = sum((m * (torch.randn(m.shape, generator=g) / 8).to(dev)).sum() for m in logits)
loss.backward()
named = sorted(model.named_parameters())
record("train forward_backbone + forward_mask + backward", [r[0].F] + list(r[3][4][0]) + logits + [p.grad for _, p in named])
digests["train grads present"] = sum(p.grad is not None for _, p in named)
print(f"train: {digests['train grads present']} of {len(named)} parameters have a gradient", flush=True)
model.zero_grad()
model.eval()
model.load_state_dict(state0)

# ---- unfused: the op program with the residual projections as separate launches
del trace[:]
with torch.no_grad():
    prog = BackboneProgram(model, dev, fuse_proj=False)
    x, raw = inputs(1)
    scene = Scene(x.C)
    y = torch.empty((len(x), model.mask_dim), dtype=torch.float32, device=dev)
    ws = prog.run(scene, x.F, y)
record("unfused BackboneProgram(fuse_proj=False) + run", [y], prog)
if args.json:
    with open(args.json, "w") as f:
        json.dump(digests, f, indent=1)
