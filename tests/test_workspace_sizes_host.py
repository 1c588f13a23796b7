"""The sizes of the session's workspaces (no GPU): every ``a3d_*_workspace_bytes`` query of the session's files against
literals.  The layouts matter across calls -- ``a3d_absorb_pieces`` and ``a3d_vote_pieces`` read what an earlier call left in
the same workspace -- and the queries are host-only functions of their arguments.

WHERE THE NUMBERS CAME FROM: each literal was printed by the library built from the commit BEFORE the one that moved the
carving of these workspaces onto one shared ``Carver`` (session_device.h), by calling the same seven functions with the same
arguments; none was taken from the code under test.  A refused size (n = -1, n = 2^31) answers 0 where the function refuses
it; ``a3d_render_workspace_bytes`` takes an int64 count of primitives and does not refuse 2^31."""
import pytest

NS = (0, 1, 63, 64, 65, 80_000, 2**31 - 1, -1, 2**31)
CAPS = ((0, 1), (0, 256), (1, 1), (1, 256), (1024, 1), (1024, 256))          # (capacity, n_classes)
VIEWS = ((1, 1), (16, 16), (17, 17), (640, 480))
PAIRS = (0, 1, 1024)                                                        # pair_capacity of a render

SESSION = 530432
PIECES = {0: 1280, 1: 1280, 63: 2304, 64: 2304, 65: 3584, 80000: 2880000, 2147483647: 77309411328, -1: 0, 2147483648: 0}
GROW = {0: 5120, 1: 5120, 63: 5376, 64: 5376, 65: 5888, 80000: 1044480, 2147483647: 27917291776, -1: 0, 2147483648: 0}
NORMALS = {0: 2816, 1: 2816, 63: 5632, 64: 5632, 65: 8448, 80000: 7040000, 2147483647: 188978561024, -1: 0, 2147483648: 0}
ABSORB = {                                                                  # n: one size per entry of CAPS
    0: (2304, 2304, 2304, 3072, 9984, 1054464),
    1: (2304, 2304, 2304, 3072, 9984, 1054464),
    63: (3328, 3328, 3328, 4096, 11008, 1055488),
    64: (3328, 3328, 3328, 4096, 11008, 1055488),
    65: (5120, 5120, 5120, 5888, 12800, 1057280),
    80000: (3520512, 3520512, 3520512, 3521280, 3528192, 4572672),
    2147483647: (94489281024, 94489281024, 94489281024, 94489281792, 94489288704, 94490333184),
    -1: (0, 0, 0, 0, 0, 0),
    2147483648: (0, 0, 0, 0, 0, 0),
}
VOTE = {
    0: (2048, 2048, 2048, 2816, 9728, 1054208),
    1: (2048, 2048, 2048, 2816, 9728, 1054208),
    63: (3072, 3072, 3072, 3840, 10752, 1055232),
    64: (3072, 3072, 3072, 3840, 10752, 1055232),
    65: (4608, 4608, 4608, 5376, 12288, 1056768),
    80000: (3200512, 3200512, 3200512, 3201280, 3208192, 4252672),
    2147483647: (85899346432, 85899346432, 85899346432, 85899347200, 85899354112, 85900398592),
    -1: (0, 0, 0, 0, 0, 0),
    2147483648: (0, 0, 0, 0, 0, 0),
}
RENDER = {                                                                  # (n_primitives, width, height): one size per entry of PAIRS
    (0, 1, 1): (1792, 1792, 5632),
    (0, 16, 16): (1792, 1792, 5632),
    (0, 17, 17): (1792, 1792, 5632),
    (0, 640, 480): (15616, 15616, 19456),
    (1, 1, 1): (1792, 1792, 5632),
    (1, 16, 16): (1792, 1792, 5632),
    (1, 17, 17): (1792, 1792, 5632),
    (1, 640, 480): (15616, 15616, 19456),
    (63, 1, 1): (2560, 2560, 6400),
    (63, 16, 16): (2560, 2560, 6400),
    (63, 17, 17): (2560, 2560, 6400),
    (63, 640, 480): (16384, 16384, 20224),
    (64, 1, 1): (2560, 2560, 6400),
    (64, 16, 16): (2560, 2560, 6400),
    (64, 17, 17): (2560, 2560, 6400),
    (64, 640, 480): (16384, 16384, 20224),
    (65, 1, 1): (3072, 3072, 6912),
    (65, 16, 16): (3072, 3072, 6912),
    (65, 17, 17): (3072, 3072, 6912),
    (65, 640, 480): (16896, 16896, 20736),
    (80000, 1, 1): (1601280, 1601280, 1605120),
    (80000, 16, 16): (1601280, 1601280, 1605120),
    (80000, 17, 17): (1601280, 1601280, 1605120),
    (80000, 640, 480): (1615104, 1615104, 1618944),
    (2147483647, 1, 1): (42949674240, 42949674240, 42949678080),
    (2147483647, 16, 16): (42949674240, 42949674240, 42949678080),
    (2147483647, 17, 17): (42949674240, 42949674240, 42949678080),
    (2147483647, 640, 480): (42949688064, 42949688064, 42949691904),
    (-1, 1, 1): (0, 0, 0),
    (-1, 16, 16): (0, 0, 0),
    (-1, 17, 17): (0, 0, 0),
    (-1, 640, 480): (0, 0, 0),
    (2147483648, 1, 1): (42949674240, 42949674240, 42949678080),
    (2147483648, 16, 16): (42949674240, 42949674240, 42949678080),
    (2147483648, 17, 17): (42949674240, 42949674240, 42949678080),
    (2147483648, 640, 480): (42949688064, 42949688064, 42949691904),
}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib.load()


def test_one_argument_workspaces(L):
    assert L.a3d_session_workspace_bytes() == SESSION
    for name, want in (("pieces", PIECES), ("grow", GROW), ("normals", NORMALS)):
        assert set(want) == set(NS)
        got = {n: getattr(L, f"a3d_{name}_workspace_bytes")(n) for n in NS}
        assert got == want, name


def test_absorb_and_vote_workspaces(L):
    for name, want in (("absorb", ABSORB), ("vote", VOTE)):
        assert set(want) == set(NS)
        fn = getattr(L, f"a3d_{name}_workspace_bytes")
        got = {n: tuple(fn(n, capacity, n_classes) for capacity, n_classes in CAPS) for n in NS}
        assert got == want, name


def test_render_workspace(L):
    assert set(RENDER) == {(n, w, h) for n in NS for w, h in VIEWS}
    got = {(n, w, h): tuple(L.a3d_render_workspace_bytes(n, w, h, cap) for cap in PAIRS) for n in NS for w, h in VIEWS}
    assert got == RENDER
