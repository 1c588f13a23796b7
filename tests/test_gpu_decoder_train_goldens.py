"""The HIP decoder training tape against the reference's own backward (tests/golden/make_decoder_train_goldens.py): one
DecoderTape (batched for a batch fixture) at the fixture's p and seed, the HIP SetCriterion.forward_and_grad, then
tape.backward, with both attention paths (train_decoder.FLASH True and False).  The attention masks must equal the
fixture's; the ReLU decisions too, except at the fixture's listed near-zero pre-activations, where the fp32 forward may
take the other branch than the float64 one: there the reference gradients are corrected by two float64 oracle runs
(fixture decisions vs tape decisions), as in test_gpu_backbone_goldens.py."""
import pytest
import torch

import decoder_train_fixture as dtf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
# tightened where the first MI355X runs sat far below decoder_train_fixture.GPU_BARS.  Observed worst over the five
# fixtures and both attention paths: logits 9.0e-7, logit sums 1.6e-7, loss 5.9e-7, parameter gradients 4.3e-4
# (mask_embed_head.2.bias, whose exact gradient is 0: rounding noise against the 1e-3 floor), d_pcd 3.5e-6, d_pcd sums 2.2e-8
BARS = dict(dtf.GPU_BARS, **{"logits": 2e-5, "logit sums": 2e-5, "loss": 5e-6, "d_pcd": 1e-4, "d_pcd sums": 1e-4})


def _model(p, decoder_weights):
    from agile3d_amd import build_model, default_args
    torch.manual_seed(0)
    model = build_model(default_args(dropout=p))
    sd = model.state_dict()
    sd.update(decoder_weights)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).train()


@pytest.mark.parametrize("flash", [True, False], ids=["flash", "dense"])
@pytest.mark.parametrize("name", dtf.names())
def test_tape_matches_the_reference_backward(name, flash, decoder_weights):
    import agile3d_amd.train_decoder as TD
    from agile3d_amd import default_args
    from agile3d_amd.criterion import build_mask_criterion
    f = dtf.load(name)
    p, seed = float(f["p"]), int(f["seed"])
    S = f["samples"]
    single = len(S) == 1
    model = _model(p, decoder_weights)
    pcds = [torch.from_numpy(s["case"]["feats128"]).to(DEV) for s in S]
    poss = [torch.from_numpy(s["case"]["pos_enc"]).to(DEV) for s in S]
    TD.FLASH = flash
    try:
        if single:
            tape = TD.DecoderTape(model, pcds[0], poss[0], S[0]["ci"], S[0]["ct"], dropout=p, seed=seed if p > 0 else None)
        else:
            tape = TD.DecoderTape(model, pcds, poss, [s["ci"] for s in S], [s["ct"] for s in S], dropout=p, seed=seed)
        logits = [[lg] if single else list(lg) for lg in tape.logits]          # [pass][sample]
        crit = build_mask_criterion(default_args(bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"]))
        outputs = {"pred_masks": logits[2], "aux_outputs": [{"pred_masks": logits[l]} for l in range(2)]}
        losses, g = crit.forward_and_grad(outputs, [s["targets"].to(DEV) for s in S], [s["weights"].to(DEV) for s in S])
        d_logits = [g["aux_outputs"][0], g["aux_outputs"][1], g["pred_masks"]]
        # the tape's branch decisions, per sample in the fixture's layout (read before the backward)
        masks = [[m] if single else list(m) for m in tape.attn_masks]
        relu = [[tape.relu_masks[j][q0:q1].cpu().double() for j in range(6)] for q0, q1 in tape.q_ranges]
        grads, d_pcd = tape.backward([d[0] for d in d_logits] if single else d_logits)
    finally:
        TD.FLASH = True
    for l in range(2):
        for b, s in enumerate(S):
            assert torch.equal(masks[l][b].cpu().bool(), s["attn_masks"][l]), (name, l, b)
    n_flip = 0
    for b, s in enumerate(S):
        for j in range(6):
            for r, c in torch.nonzero(relu[b][j] != s["relu"][j]).tolist():
                assert (j, r, c) in s["near"], (name, b, j, r, c)
                n_flip += 1
    delta = None
    if n_flip:
        own, hip = dtf.oracle_run(f, decoder_weights), dtf.oracle_run(f, decoder_weights, relu=relu)
        delta = dict(grads={k: hip["grads"][k] - own["grads"][k] for k in own["grads"]},
                     d_pcd=[h - o for h, o in zip(hip["d_pcd"], own["d_pcd"])])
    n0 = [r0 for r0, _ in tape.n_ranges]
    got = dict(logits=[[logits[l][b].cpu().double() for l in range(3)] for b in range(len(S))],
               losses={k: v.item() for k, v in losses.items()},
               d_pcd=[d_pcd[a:a + s["N"]].cpu().double() for a, s in zip(n0, S)],
               grads={k: v.cpu().double() for k, v in grads.items()})
    got["losses"]["total"] = sum(got["losses"][k] * dtf.WEIGHT_DICT[k] for k in got["losses"])
    worst = dtf.errors(f, got, delta)
    dtf.report(f"HIP tape vs reference, {name} ({'flash' if flash else 'dense'}, p = {p}, {n_flip} ReLU decisions at a kink "
               f"corrected)", worst, BARS)
    for q, (v, where) in worst.items():
        assert v <= BARS[q], (name, q, v, where)
