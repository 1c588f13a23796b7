"""No GPU: ``modules.walk_res16unet34c`` -- the one statement of the Res16UNet34C wiring that ``engine.BackboneProgram`` and
``train_backbone.BackboneTape`` both build from -- through a builder that only records (verb, level, cin, cout, modules)."""
import torch

from agile3d_amd.modules import Res16UNet34CParams, SparseConvParams, walk_res16unet34c


class Recorder:
    """Activations are (level, channels); a concatenation buffer remembers what was written into its halves."""

    def __init__(self, bb, head):
        self.names = {id(m): "backbone." + n for n, m in bb.named_modules()}
        self.names[id(head)] = "lin_squeeze_head"
        self.log, self.cats = [], []

    def _rec(self, verb, level, cin, cout, *modules):
        self.log.append((verb, level, cin, cout, tuple(self.names[id(m)] for m in modules)))

    def concat_buffer(self, level, c_up, c_skip):
        self.cats.append({"level": level, "c_up": c_up, "c_skip": c_skip, "up": None, "skip": None})
        return self.cats[-1]

    def stem(self, conv, bn, cat):
        self._rec("stem", 0, conv.cin, conv.cout, conv, bn)
        cat["skip"] = (0, conv.cout)
        return cat["skip"]

    def down(self, conv, bn, x):
        assert x[1] == conv.cin
        self._rec("down", x[0], conv.cin, conv.cout, conv, bn)
        return x[0] + 1, conv.cout

    def layer(self, blocks, x, skip_of=None):
        level, c = x
        for blk in blocks:
            assert blk.conv1.cin == c and (blk.downsample is None) == (c == blk.conv1.cout)
            self._rec("block", level, c, blk.conv2.cout, blk)
            c = blk.conv2.cout
        if skip_of is not None:
            assert skip_of["level"] == level and skip_of["skip"] is None
            skip_of["skip"] = (level, c)
        return level, c

    def up(self, conv, bn, x, cat):
        assert x == (cat["level"] + 1, conv.cin) and cat["up"] is None
        self._rec("up", x[0], conv.cin, conv.cout, conv, bn)
        cat["up"] = (cat["level"], conv.cout)

    def concat(self, cat):
        # both halves written, at this level, of the widths the buffer was made with: the skip is the LAST c_skip columns
        assert cat["up"] == (cat["level"], cat["c_up"]) and cat["skip"] == (cat["level"], cat["c_skip"])
        self._rec("concat", cat["level"], cat["c_up"], cat["c_skip"])
        return cat["level"], cat["c_up"] + cat["c_skip"]

    def head(self, conv, x):
        assert x == (0, conv.cin)
        self._rec("head", 0, conv.cin, conv.cout, conv)


def _walk():
    torch.manual_seed(0)
    bb = Res16UNet34CParams()
    head = SparseConvParams(bb.PLANES[7], 128, 1, bias=True)
    rec = Recorder(bb, head)
    return bb, head, rec, walk_res16unet34c(bb, head, rec)


def test_every_parameter_is_visited_by_exactly_one_step():
    """What ``BackboneTape.backward(on_grad=...)`` assumes: a parameter's gradient is final after one step."""
    bb, head, rec, _ = _walk()
    modules = dict(bb.named_modules(prefix="backbone"), lin_squeeze_head=head)
    seen = [id(p) for *_, names in rec.log for n in names for p in modules[n].parameters()]
    everything = [id(p) for p in list(bb.parameters()) + list(head.parameters())]
    assert len(seen) == len(set(seen)) and sorted(seen) == sorted(everything)


def test_order_and_counts_of_the_steps():
    bb, _, rec, _ = _walk()
    verbs = [e[0] for e in rec.log]
    assert verbs.count("down") == 4 and verbs.count("up") == 4 and verbs.count("concat") == 4
    assert verbs[0] == "stem" and verbs[-1] == "head" and verbs.count("stem") == verbs.count("head") == 1
    # stem, (down, layer) x 4, (up, concat, layer) x 4, head -- with the block counts of LAYERS
    runs = [v for i, v in enumerate(verbs) if v != "block" or verbs[i - 1] != "block"]
    assert runs == ["stem"] + ["down", "block"] * 4 + ["up", "concat", "block"] * 4 + ["head"]
    blocks = [e for e in rec.log if e[0] == "block"]
    per_layer = [sum(e[4][0].startswith(f"backbone.block{k}.") for e in blocks) for k in range(1, 9)]
    assert tuple(per_layer) == bb.LAYERS
    assert [e[4][0] for e in blocks] == [f"backbone.block{k}.{i}" for k in range(1, 9) for i in range(bb.LAYERS[k - 1])]
    assert [e[1] for e in rec.log if e[0] == "down"] == [0, 1, 2, 3] and [e[1] for e in rec.log if e[0] == "up"] == [4, 3, 2, 1]
    assert [e[4] for e in rec.log if e[0] in ("down", "up")] == [
        ("backbone.conv1p1s2", "backbone.bn1"), ("backbone.conv2p2s2", "backbone.bn2"), ("backbone.conv3p4s2", "backbone.bn3"),
        ("backbone.conv4p8s2", "backbone.bn4"), ("backbone.convtr4p16s2", "backbone.bntr4"), ("backbone.convtr5p8s2", "backbone.bntr5"),
        ("backbone.convtr6p4s2", "backbone.bntr6"), ("backbone.convtr7p2s2", "backbone.bntr7")]


def test_concatenations_put_the_skip_last_at_the_widths_of_the_kernels():
    bb, _, rec, _ = _walk()
    P = bb.PLANES
    assert [(c["level"], c["c_up"], c["c_skip"]) for c in rec.cats] == [(0, P[7], 32), (1, P[6], P[0]), (2, P[5], P[1]), (3, P[4], P[2])]
    concats = [e for e in rec.log if e[0] == "concat"]
    assert [e[1] for e in concats] == [3, 2, 1, 0]
    for (_, level, c_up, c_skip, _), k in zip(concats, (5, 6, 7, 8)):
        first = getattr(bb, f"block{k}")[0]
        # the layer that reads the concatenation takes c_up + c_skip channels; the transposed conv wrote the first c_up
        assert first.conv1.kernel.shape[1] == c_up + c_skip and first.downsample[0].kernel.shape[0] == c_up + c_skip
        assert getattr(bb, f"convtr{k - 1}p{2 ** (9 - k)}s2").kernel.shape[2] == c_up
    # the skips: the stem's output and the outputs of block1..3, each written before the decoder reads it
    log_names = [e[4][0] if e[4] else "" for e in rec.log]
    for level, writer in enumerate(["backbone.conv0p1s1", "backbone.block1.1", "backbone.block2.2", "backbone.block3.3"]):
        reader = [i for i, e in enumerate(rec.log) if e[0] == "concat" and e[1] == level][0]
        assert log_names.index(writer) < reader


def test_the_five_feature_maps():
    bb, _, _, fms = _walk()
    P = bb.PLANES
    assert fms == [(4, P[3]), (3, P[4]), (2, P[5]), (1, P[6]), (0, P[7])]
