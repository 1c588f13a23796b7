#!/usr/bin/env python3
"""Digests of the interactive loop's host module (agile3d_amd/clicks.py) on seeded inputs, to compare two commits: sha256 of
what every public function returns, and of the trace -- the ordered list of (symbol, every argument that is not a pointer)
-- of the library calls behind the batched functions and behind one session.  Sections:
  golden   every public function over the cases of tests/golden/clicks_cases.npz, per sample and as one batch
  prune    the search's stress cases (tests/test_gpu_clicks.py: _prune_cases) up to 70 k points, per sample and as one batch
  rounds   Evaluate on four 3000-voxel scenes in lock-step (2 objects, max_num_clicks 2: rounds 0, 2, 3, 4)
  session  InteractiveSession.infer() and guide() on one scene
Only public names of clicks.py, evaluate.py and session.py and setattr on the loaded library's symbols are used, so the same
file runs on either commit:
  python tools/click_round_digest.py [--json digests.json]"""
import argparse, ctypes, hashlib, json, os, random, sys, tempfile, types
import numpy as np
import torch
import lib_trace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from agile3d_amd import build_model, clicks as pc, default_args, randomize_bn_stats
from agile3d_amd.evaluate import Evaluate
from agile3d_amd.session import InteractiveSession
from agile3d_amd.synthetic import make_scene

ap = argparse.ArgumentParser()
ap.add_argument("--json", default="", help="write {section: sha256 or call count} here")
args = ap.parse_args()


def plain(v):
    """A result as something with a stable repr: tensors and arrays as the sha256 of their bytes, floats by their bits."""
    if torch.is_tensor(v):
        v = v.detach().contiguous().cpu().numpy()
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, dict):
        return [(str(k), plain(x)) for k, x in v.items()]
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return np.float64(v).tobytes().hex()
    if isinstance(v, ctypes.Structure):
        return tuple(plain(getattr(v, f[0])) for f in v._fields_)
    return getattr(v, "value", v)


trace = lib_trace.install(plain)

digests = {}


def record(section, value, with_trace=False):
    digests[section] = hashlib.sha256(repr(plain(value)).encode()).hexdigest()
    line = f"{section} | values {digests[section][:16]}"
    if with_trace:
        digests[section + " trace"] = lib_trace.digest(trace)
        digests[section + " calls"] = len(trace)
        line += f" | trace {digests[section + ' trace'][:16]} [{len(trace)} calls]"
        for t in trace:
            print("    call", *t)
    print(line, flush=True)
    del trace[:]


t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

# ---- golden: every public function over the reference's cases
G = np.load(os.path.join(ROOT, "tests", "golden", "clicks_cases.npz"))
names = [str(n) for n in G["names"]]
xs, labs, prs = ([t(G[f"{n}/{k}"]) for n in names] for k in ("xyz", "labels", "pred"))
gen = torch.Generator().manual_seed(0)
logits = [torch.randn(len(l), 3 + i, generator=gen).cuda() for i, l in enumerate(labs)]
clicks = [{"0": [0, len(l) // 2], "1": [len(l) - 1, 0], "2": []} for l in labs]
invs = [t(np.random.default_rng(i).integers(0, len(l), 2 * len(l))) for i, l in enumerate(labs)]
labs_full = [l[m] for l, m in zip(labs, invs)]
record("golden argmax_labels", [pc.argmax_labels(lg, ck) for lg, ck in zip(logits, clicks)] + [pc.argmax_labels(logits[0])])
record("golden argmax_labels_batch", pc.argmax_labels_batch(logits, clicks), True)
record("golden iou_counts", [pc.iou_counts(p, l) for p, l in zip(prs, labs)] + [pc.iou_counts(p, l, m, 16) for p, l, m in zip(prs, labs_full, invs)])
record("golden iou_counts_batch", [pc.iou_counts_batch(prs, labs), pc.iou_counts_batch(prs, labs_full, invs, 16)], True)
record("golden mean_iou_scene", [pc.mean_iou_scene(p, l) for p, l in zip(prs, labs)] + [pc.mean_iou_scene(p, l, m) for p, l, m in zip(prs, labs_full, invs)])
record("golden mean_iou_scene_batch", [pc.mean_iou_scene_batch(prs, labs), pc.mean_iou_scene_batch(prs, labs_full, invs)], True)
record("golden error_clusters", [pc.error_clusters(p, l, x) for p, l, x in zip(prs, labs, xs)])
record("golden error_clusters_batch", pc.error_clusters_batch(prs, labs, xs), True)
record("golden mean_iou_and_clusters_batch", pc.mean_iou_and_clusters_batch(prs, labs_full, invs, labs, xs), True)
for mode, (cur, training) in {"eval0": (0, False), "evalk": (7, False), "train": (None, True)}.items():
    p_mode = [torch.zeros(len(l), device="cuda") for l in labs] if mode == "eval0" else prs
    random.seed(123)
    record(f"golden get_simulated_clicks {mode}", [pc.get_simulated_clicks(p, l.long(), x, cur, training=training) for p, l, x in zip(p_mode, labs, xs)])
    random.seed(123)
    record(f"golden get_simulated_clicks_batch {mode}", pc.get_simulated_clicks_batch(p_mode, [l.long() for l in labs], xs, cur, training=training), True)
    random.seed(123)
    record(f"golden pick_clicks_batch {mode}", pc.pick_clicks_batch(pc.error_clusters_batch(p_mode, labs, xs), labs, xs, cur, training=training,
                                                                  num_objs=[int((torch.unique(l) != 0).sum()) for l in labs]))
cur_c, cur_t = {"0": [1], "1": [2, 3]}, {"0": [0], "1": [1, 2]}
record("extend_clicks", pc.extend_clicks(cur_c, cur_t, {"1": [9], "0": [4]}, {"1": [0], "0": [1]}))
sizes = [len(l) for l in labs]
ranges = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
bidx = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(sizes)]).cuda()
record("golden cal_click_loss_weights", [pc.cal_click_loss_weights(bidx, torch.cat(xs), labs, clicks),
                                         pc.cal_click_loss_weights(bidx, torch.cat(xs), labs, clicks, ranges=ranges)])

# ---- prune: the bounded search's stress cases, per sample and as one batch (the spatial order from 20 k points on)
import test_gpu_clicks as T
cases = [c for c in T._prune_cases() if len(c[2]) <= 70_001]
cp, cl, cx = ([t(c[k]) for c in cases] for k in range(3))
record("prune error_clusters", [pc.error_clusters(p, l, x) for p, l, x in zip(cp, cl, cx)])
record("prune error_clusters_batch", pc.error_clusters_batch(cp, cl, cx), True)
record("prune error_clusters_batch, second round (orders cached)", pc.error_clusters_batch(cp, cl, cx), True)

# ---- rounds: Evaluate's lock-step loop on four scenes
torch.manual_seed(0)
model = randomize_bn_stats(build_model(default_args())).eval().cuda()
coords, raw, feats, labels, num_obj, scene_names = [], [], [], [], [], []
for i in range(4):
    sc = make_scene(3000, seed=20 + i)
    ids = sorted((j for j in np.unique(sc["labels"]) if j > 0), key=lambda j: -(sc["labels"] == j).sum())[:2]
    lab = np.zeros(len(sc["coords"]), np.int64)
    for k, j in enumerate(ids, start=1):
        lab[sc["labels"] == j] = k
    c = sc["coords"].copy()
    c[:, 0] = i
    coords.append(torch.from_numpy(c)); raw.append(torch.from_numpy(sc["raw_xyz"])); feats.append(torch.from_numpy(sc["feats"]))
    labels.append(torch.from_numpy(lab)); num_obj.append(2); scene_names.append(f"scene{i:04d}_00")
batch = (torch.cat(coords), torch.cat(raw), torch.cat(feats), labels, [l.clone() for l in labels],
         [torch.arange(len(l)) for l in labels], [{str(k): [] for k in range(3)} for _ in labels], scene_names, num_obj)
seen = []
random.seed(9)
with tempfile.TemporaryDirectory() as tmp:
    ev = types.SimpleNamespace(output_dir=tmp, max_num_clicks=2, val_list=None)
    csv = Evaluate(model, [batch], ev, torch.device("cuda"),
                   lambda idx, cur, pred, iou, ci, ct: seen.append((idx, cur, pred.clone(), iou.clone(), {k: list(v) for k, v in ci.items()},
                                                                    {k: list(v) for k, v in ct.items()})))
    rows = open(csv).read()
trace[:] = [c for c in trace if c[0].startswith(("a3d_argmax", "a3d_iou", "a3d_click"))]
record("rounds Evaluate (4 scenes, rounds 0 2 3 4)", [seen, rows], True)

# ---- session: infer() and guide() on one scene
sc = make_scene(3000, seed=3, voxel_size=0.02)
xyz, lab = sc["raw_xyz"].astype(np.float32), sc["labels"].astype(np.int32)
torch.manual_seed(0)
model2 = randomize_bn_stats(build_model(default_args(voxel_size=0.02))).eval().cuda()
ses = InteractiveSession(model2, voxel_size=0.02)
ses.load_scene(xyz, sc["feats"].astype(np.float32), lab, name="digest")
inst = [i for i in np.unique(lab) if i > 0][:3]
for k, i in enumerate(inst):
    ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
ses.click(xyz[np.flatnonzero(lab == 0)[0]] if (lab == 0).any() else xyz[0], 0)
del trace[:]
res = ses.infer()
g = ses.guide()
record("session infer + guide", [res.labels_full, res.colors, res.miou, res.iou_per_object, g.labels_qv, g.runner_qv, g.margin_qv, g.colors,
                                 g.suggestions, g.object_contested], True)
g2 = ses.guide(regions="connected")
record('session guide(regions="connected")', [g2.suggestions, g2.n_spots, g2.n_spots_searched], True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(digests, f, indent=1)
