"""The decoder oracle's training graph against the reference's own backward (tests/golden/make_decoder_train_goldens.py:
float64 training-mode forward_mask, SetCriterion with bce + dice and the aux levels, loss.backward()).  oracle/decoder.py
with grad=True, under the fixture's attention masks and ReLU decisions and, at p > 0, with its dropout hook keyed like
the fixture, must reproduce every stored loss, logit, parameter gradient and dL/d(pcd_features) entry.  Negative
controls: each mutation of the graph or of the dropout placement must miss the fixtures by at least 100x the bars of the
HIP tape (decoder_train_fixture.GPU_BARS)."""
import math

import pytest
import torch

import decoder_train_fixture as dtf
from oracle import decoder as od

TOL = 1e-9          # both sides float64; observed <= 1.2e-12 (parameter gradients), <= 3e-15 elsewhere
CONTROL_MISS = 100.0


@pytest.mark.parametrize("name", dtf.names())
def test_oracle_reproduces_the_reference_backward(name, decoder_weights):
    f = dtf.load(name)
    run = dtf.oracle_run(f, decoder_weights)
    worst = dtf.errors(f, run)
    dtf.report(f"oracle vs reference, {name} (p = {float(f['p'])})", worst)
    assert all(v <= TOL for v, _ in worst.values()), worst
    # the oracle's own ReLU decisions are the fixture's wherever the pre-activation is not listed as near zero
    for s, own in zip(f["samples"], dtf.decisions(run, f)):
        for j, (a, b) in enumerate(zip(s["relu"], own)):
            for r, c in torch.nonzero(a != b).tolist():
                assert (j, r, c) in s["near"], (name, j, r, c)


def test_fixtures_cover_the_issue_cases():
    cover = {n: dtf.load(n) for n in dtf.names()}
    assert set(cover) == {"q75", "q205", "dup", "drop", "batch2"}
    assert max(s["Q"] for s in cover["q205"]["samples"]) == 205 and cover["q75"]["samples"][0]["Q"] == 75
    dup = cover["dup"]["samples"][0]
    assert dup["ci"]["0"] == [] and int((dup["targets"] == 1).sum()) == 0      # learned bg queries only, an empty label
    assert float(cover["drop"]["p"]) == 0.1 and float(cover["batch2"]["p"]) == 0.5
    b2 = cover["batch2"]["samples"]
    assert len(b2) == 2 and all(len(s["ci"]["0"]) > 0 for s in b2)
    # the stored ReLU decisions and the listed near-zero inputs agree
    for f in cover.values():
        for s in f["samples"]:
            for (j, r, c), v in s["near"].items():
                assert abs(v) < 1e-3 and s["relu"][j][r, c] == float(v > 0)


def _miss(f, run):
    worst = dtf.errors(f, run)
    ratio = max((v / dtf.GPU_BARS[q], q) if not math.isnan(v) else (math.inf, q) for q, (v, _) in worst.items())
    return worst, ratio


def _mha_scores_dropped(sd, prefix, query, key, value, attn_mask=None, nhead=8, drop=None, site=None):
    """oracle.decoder.mha with the mutation: the dropout mask applied to the scores before the softmax."""
    E = query.shape[-1]
    W, b = sd[prefix + "in_proj_weight"], sd[prefix + "in_proj_bias"]
    q = (query @ W[:E].T + b[:E]).reshape(-1, nhead, E // nhead).transpose(0, 1) / math.sqrt(E // nhead)
    k = (key @ W[E:2 * E].T + b[E:2 * E]).reshape(-1, nhead, E // nhead).transpose(0, 1)
    v = (value @ W[2 * E:].T + b[2 * E:]).reshape(-1, nhead, E // nhead).transpose(0, 1)
    s = q @ k.transpose(1, 2)
    if drop is not None:
        s = drop(site, s)
    if attn_mask is not None:
        s = s.masked_fill(attn_mask.unsqueeze(0), float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(-1, E)
    return o @ sd[prefix + "out_proj.weight"].T + sd[prefix + "out_proj.bias"]


def _group_mean(prods):
    return prods.mean(dim=-1, keepdim=True)


CONTROLS = {
    "queries detached from pcd_features": (["q75", "q205", "dup"], dict(detach_queries=True), None),
    "FFN dropout sites 4 and 5 swapped": (["drop", "batch2"], dict(site_of=lambda s: {4: 5, 5: 4}.get(s, s)), None),
    "attention dropout on the scores before the softmax": (["drop", "batch2"], {}, ("mha", _mha_scores_dropped)),
    "sample index 0 for both samples": (["batch2"], dict(samples=[0, 0]), None),
    "group max replaced by a mean": (["q75", "dup", "drop"], {}, ("GROUP_MAX", _group_mean)),
}


@pytest.mark.parametrize("control", list(CONTROLS))
def test_negative_controls_miss_the_fixtures(control, decoder_weights):
    fixtures, kw, patch = CONTROLS[control]
    for name in fixtures:
        f = dtf.load(name)
        saved = getattr(od, patch[0]) if patch else None
        if patch:
            setattr(od, patch[0], patch[1])
        try:
            run = dtf.oracle_run(f, decoder_weights, **kw)
        finally:
            if patch:
                setattr(od, patch[0], saved)
        worst, (ratio, q) = _miss(f, run)
        print(f"negative control '{control}' on {name}: misses by {ratio:.3g}x the GPU bar ({q}: {worst[q][0]:.3e} "
              f"[{worst[q][1]}])")
        assert ratio >= CONTROL_MISS, (control, name, ratio, q)
