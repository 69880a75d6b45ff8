"""Marching cubes at the shapes that steer its kernels (meshing.hip): the soup, the edge keys, the welded and filtered
meshes and the vertex colours, byte for byte against the oracle and the numpy restatements -- never against another call
of the kernels themselves.  The shapes and fills are tests/mesh_volumes.py's; tests/test_mesh_volumes_cpu.py shows on
the CPU that every chunk and every counting workgroup of them carries surface, which is what makes a skipped workgroup,
a lost scan carry or a misplaced chunk visible here.  No tolerance appears anywhere: shapes first, then tobytes().

What fails here if meshing.hip were wrong (argued from the code, not run), and what the older oracle comparisons -- fused
spheres at (32, 32, 32), (30, 22, 37), (64, 48, 40), (40, 36, 32), random signs at 66 x 7 x 5, the 512^3 background --
see of it:
  logical_block with band = max(1, wpp / 8)   column 8 of (130, 140, 30) (wpp 9), likewise wpp 10 and 11, is never
      counted: vertices missing.  The older shapes have wpp 1 and 32, where both roundings agree.
  col <= wpp in place of col < wpp            where wpp is no multiple of 8 a workgroup is counted twice.  Its totals are
      written twice with the same value and its chunks listed twice, which the emit repeats harmlessly while list[] has
      room -- the spheres' case.  Here every chunk is listed, so from (2, 130, 40) on list[] runs over into listCount.
  before = carry dropped in k_mesh_scan       workgroups 1024.. of (160, 128, 104) write over the first ones.  The 512^3
      mesh sees it too, in 32-chunk mode, and was the only one.
  chunks_for's threshold in chunk_slot only   `>` reads the wrong blockSums at (256, 256, 256), `>= 2^24 - 1` at
      (273, 241, 255).  The older 256^3 volumes are compared with the level-1 call only, which shares chunk_slot.
  the emit loop without its stride            (160, 128, 104) lists over 8000 chunks (asserted on the CPU), the grid has
      4096 workgroups: the rest stays zero.  Nothing asserts how long the 512^3 list is.
  nx >= 9 in place of nx >= 64                (9, 96, 130) and (63, 7, 40): lanes past the second row keep x >= nx.  The
      older shapes with nx = 30, 32, 40 see that as well.
  g[r] == 255 in place of g[r] != 0           the masked variants hold bytes 1, 2 and 128; the older masks are 0 / 255.
  w[r] >= 0.f in place of w[r] > 0.f          a tenth of the weights is 0.0, -0.0 or -1.0 (the last tells >= from no
      test).  Fused volumes, whose unobserved voxels meet negative ones, most likely see it too.
  color_cube without the c[0].w == 0 rule     an edge from an uncoloured to a coloured voxel turns black: two ninths of
      the vertices of every colour case.  The older colour tests compare the SET of colours or the kernel with itself."""
import numpy as np
import pytest

from tests import mesh_volumes as MV
from tests.components_reference import components, filter_mesh
from tests.mesh_color_reference import vertex_colours
from tests.parity_util import to_dev
from tests.weld_reference import edge_keys, weld

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "masked", "grads")   # no mask; the foreground mask; a materialised gradient volume
SOUP_CASES = ([("dense", s, v) for s in MV.DENSE_SMALL for v in VARIANTS] +
              [("dense", MV.CARRY, v) for v in VARIANTS[:2]] + [("sparse", s, "plain") for s in MV.SPARSE])
# the table: every dense case below the carry case, the variants in turn, and a 32-chunk volume among them
TABLE = [("dense", s, VARIANTS[k % 3]) for k, s in enumerate(MV.DENSE_SMALL)] + [("sparse", MV.SPARSE[2], "plain")]
KEY_CASES = ([("dense", s, v) for s in MV.DENSE for v in VARIANTS[:2]] + [("sparse", MV.SPARSE[1], "plain")])
FILTER_CASES = [("dense", s, v) for s, v in zip(MV.FILTERED, ("masked", "plain", "plain", "masked"))]
COLOUR_CASES = [("dense", s, v) for s, v in zip(MV.COLOURED, ("plain", "plain", "masked"))]


def case_id(c):
    return f"{c[0]}-{MV.name_of(c[1])}-{c[2]}"


@pytest.fixture(scope="module")
def ops(dev):
    from emfusion_amd import ops
    return ops


_host, _soup, _dev = {}, {}, {}


def host(oracle, case):
    """(tsdf, weights, fg or None, grads or None, voxel size) on the host."""
    if case not in _host:
        kind, shape, variant = case
        t, w, fg, vox = MV.dense(shape) if kind == "dense" else MV.sparse(shape)
        _host[case] = (t, w, fg if variant == "masked" else None,
                       oracle.compute_tsdf_grads(t) if variant == "grads" else None, vox)
    return _host[case]


def soup(oracle, case):
    """The oracle's mesh of the case: computed once, shared, left unchanged."""
    if case not in _soup:
        t, w, fg, grads, vox = host(oracle, case)
        kw = {k: v for k, v in (("fg", fg), ("grads", grads)) if v is not None}
        _soup[case] = oracle.marching_cubes(t, w, vox, **kw)
    return _soup[case]


def volume(oracle, case):
    """The case as extract_meshes takes it (uploaded once; extract_mesh takes the same arrays)."""
    if case not in _dev:
        t, w, fg, grads, vox = host(oracle, case)
        _dev[case] = dict(tsdf=to_dev(t), weights=to_dev(w), voxel_size=vox, fg_mask=None if fg is None else to_dev(fg),
                          grads=None if grads is None else to_dev(grads))
    return _dev[case]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d in (_host, _soup, _dev):
        d.clear()


def level1(ops, v, **kw):
    return ops.extract_mesh(v["tsdf"], v["weights"], v["voxel_size"], fg_mask=v["fg_mask"], grads=v["grads"], **kw)


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k)


@pytest.mark.parametrize("case", SOUP_CASES, ids=case_id)
def test_soup_equals_the_oracle(oracle, ops, case):
    want = soup(oracle, case)
    assert len(want[0]) > 100 and len(want[2]) > 50
    same(level1(ops, volume(oracle, case)), want, case_id(case))


def test_table_slices_equal_the_oracle(oracle, ops):
    """One launch over 8-chunk and 32-chunk models: every slice against the oracle's mesh of that volume alone, in the
    listed order and in a permutation."""
    vols = [volume(oracle, c) for c in TABLE]
    for order in (np.arange(len(TABLE)), np.random.default_rng(252).permutation(len(TABLE))):
        got = ops.extract_meshes([vols[i] for i in order])
        assert len(got) == len(TABLE)
        for k, i in enumerate(order):
            same(got[k], soup(oracle, TABLE[i]), (k, case_id(TABLE[i])))


@pytest.mark.parametrize("case", KEY_CASES, ids=case_id)
def test_edge_keys_equal_the_restatement(oracle, ops, case):
    t, w, fg, grads, vox = host(oracle, case)
    want = edge_keys(t, w, fg)
    assert len(want) > 100
    v = volume(oracle, case)
    got = ops.mesh_edge_keys(v["tsdf"], v["weights"], fg_mask=v["fg_mask"])
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("case", FILTER_CASES, ids=case_id)
def test_welded_and_filtered_meshes_equal_the_restatements(oracle, ops, case):
    """Dense random signs: tens of thousands of tiny components beside a few large ones."""
    t, w, fg, grads, vox = host(oracle, case)
    welded = weld(*soup(oracle, case), edge_keys(t, w, fg))
    v = volume(oracle, case)
    same(level1(ops, v, weld=True), welded, case_id(case))
    comps = components(welded[2], len(welded[0]))
    for kw in (dict(min_triangles=8), dict(largest_only=True)):
        want = filter_mesh(*welded, comps=comps, **kw)
        assert 0 < len(want[0]) < len(welded[0]) and 0 < len(want[2]) < len(welded[2])
        same(level1(ops, v, weld=True, **kw), want, (case_id(case), kw))


_colour = {}


def coloured(oracle, case):
    """(device colour volume, the restatement's vertex colours) of a case."""
    if case not in _colour:
        t, w, fg, grads, vox = host(oracle, case)
        col = MV.colours(case[1])
        _colour[case] = (to_dev(col), vertex_colours(t, w, col, fg))
    return _colour[case]


@pytest.mark.parametrize("case", COLOUR_CASES, ids=case_id)
def test_vertex_colours_equal_the_restatement(oracle, ops, case):
    col, want = coloured(oracle, case)
    packed = want.astype(np.uint32) @ np.array([65536, 256, 1], np.uint32)
    assert len(want) == len(soup(oracle, case)[0]) and len(np.unique(packed)) > 100
    got = level1(ops, volume(oracle, case), color=col)
    same(got[:3], soup(oracle, case), case_id(case))
    same(got[3:], (want,), case_id(case))


def test_vertex_colours_in_the_table(oracle, ops):
    """The three coloured cases and one without a colour volume (black) in one launch, largest first."""
    cases = [COLOUR_CASES[2], COLOUR_CASES[0], ("dense", (65, 7, 40), "plain"), COLOUR_CASES[1]]
    vols = []
    for c in cases:
        vols.append(dict(volume(oracle, c), color=coloured(oracle, c)[0] if c in COLOUR_CASES else None))
    got = ops.extract_meshes(vols)
    for k, c in enumerate(cases):
        same(got[k][:3], soup(oracle, c), (k, case_id(c)))
        want = coloured(oracle, c)[1] if c in COLOUR_CASES else np.zeros((len(got[k][0]), 3), np.uint8)
        same(got[k][3:], (want,), (k, case_id(c)))
    _colour.clear()
