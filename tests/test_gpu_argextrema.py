"""histogram_argextrema on the MI355X: all four outputs against tests/argextrema_oracle.py — positions exactly, values bit
for bit — and vmin / vmax bit for bit against core.histogram_extrema on the same inputs.

Every case that names a launch variant predicts the describe() line from `predict`, a restatement of choose_values /
values_geometry (xhist_values.hip.h) with the statistic's slots: 16 then 32 bytes a bin, 8 then 24 for the fast family on
float32 values, the larger pass deciding for both.  Between them the cases launch all 20 kernels the statistic adds
(argext_fast x 12, argext_generic x 6, argext_prepare, argext_finalize); the closing census of a whole -m gpu session holds
them to that.

Values are small integers (and a few special values), so that almost every bin's extreme is held by many samples: a wrong
"first" shows."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import argextrema_oracle as ao
import extrema_oracle as eo
from oracle.oracle_np import normalise_axis
from test_gpu_census import edges_of
from test_gpu_extrema import SPECIAL
from test_gpu_parity import _plan_for, xh  # noqa: F401  (xh: the module fixture)
from test_gpu_values_census import LDS_MAX, _domain_edges, _last, float_samples, int_samples, table_bytes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
SLOT, SLOT32 = (16, 32), (8, 24)  # a bin's LDS slot in pass 1 and pass 2: 64-bit keys / the fast family on float32 values


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice, restated
# ---------------------------------------------------------------------------------------------------------------------
def predict(cus, edges, cmp, sdt, vdt, n_rows, n_cols, fine=True, arith=False, layout_fast=True):
    """the describe() fields of histogram_argextrema on this input.  fine: the edges put at most two edges into a bucket of the
    fine grid (True), or exactly that many (1 / 2), or more (False); arith: the plan finds them arithmetic; layout_fast: unit
    column strides (or one column) for samples and values"""
    D = len(edges)
    n_bins = int(np.prod([len(e) - 1 for e in edges]))
    f32 = np.dtype(sdt) == F32
    out = dict(D=D, cmp=cmp, scan=0)
    fast_ok = (cmp == 0 and D <= 2 and np.dtype(sdt) in (np.dtype(F64), np.dtype(F32)) and np.dtype(vdt) == np.dtype(sdt)
               and n_bins < (1 << 24) and layout_fast)
    lds_bytes = None
    if fast_ok:
        b = SLOT32 if f32 else SLOT
        tb_fine = table_bytes(edges, "fine32" if f32 else "fine64")
        tb = None
        if fine and tb_fine + n_bins * max(b) <= LDS_MAX:
            tb, out["scan"] = tb_fine, "fine" if fine is True else fine
        elif arith and n_bins * max(b) <= LDS_MAX:
            tb, out["scan"] = 0, 5
        if tb is not None:
            out.update(family="fast", slots="lds", tables_in_lds=1)
            lds_bytes = [tb + n_bins * k for k in b]
    if lds_bytes is None:
        tb = table_bytes(edges, "native")
        til = tb + 1024 <= LDS_MAX
        lds = til and n_bins < (1 << 24) and tb + n_bins * max(SLOT) <= LDS_MAX
        out.update(family="generic", slots="lds" if lds else "global", tables_in_lds=int(til))
        lds_bytes = [(tb + (n_bins * k if lds else 0)) if til else 0 for k in SLOT]
    fast = out["family"] == "fast"
    block = 256 if fast else 512
    per_tile = block * (4 * (4 if f32 else 2) if D == 1 else 8) if fast else block
    tiles = -(-n_cols // per_tile)
    segs = []
    for lds in lds_bytes:  # (the residency is each pass's own: pass 1's slots are smaller)
        bpc = 2048 // block
        if lds:
            bpc = max(1, min(bpc, 160 * 1024 // lds))
        sg = max(1, min(tiles, -(-cus * bpc // n_rows)))
        segs.append(max(sg, -(-(tiles * per_tile) // (1 << 31))))
    out.update(block=block, segs=segs, lds_bytes=lds_bytes)
    return out


def parse(desc):
    assert desc.startswith("argextrema "), desc
    kv = dict(re.findall(r"(\w+)=(\S+)", desc))
    fam = kv["pass1"].replace("extrema_", "")
    assert kv["pass2"] == "argext_" + fam, desc
    homes = re.findall(r"slots=(\S+)", desc)
    assert len(homes) == 2 and homes[0] == homes[1], desc
    return dict(family=fam, slots=homes[0], scan=int(kv["scan"]), block=int(kv["block"]), segs=[int(t) for t in kv["segs"].split("/")],
                tables_in_lds=int(kv["tables_in_lds"]), D=int(kv["D"]), cmp=int(kv["cmp"]),
                lds_bytes=[int(t) for t in kv["lds_bytes"].split("/")])


def assert_variant(desc, want):
    got = parse(desc)
    w = dict(want)
    if w["scan"] == "fine":
        assert got["scan"] in (1, 2), (desc, want)
        w["scan"] = got["scan"]
    assert got == w, "landed elsewhere:\n  got  %s\n  want %s\n  (%s)" % (got, w, desc)
    return got


def _cus():
    from xhistogram_amd import _native

    return _native.device_info(0)["compute_units"]


# ---------------------------------------------------------------------------------------------------------------------
# data and the check
# ---------------------------------------------------------------------------------------------------------------------
def tie_values(rng, shape, dt):
    """small integers in `dt` (ties everywhere); floats also carry NaN, both zeros, infinities and subnormals"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.random(shape) < 0.5
    v = rng.integers(-3, 4, shape)
    if dt.kind != "f":
        return (v if dt.kind == "i" else v + 3).astype(dt)
    v = v.astype(F64)
    flat = v.reshape(-1)
    sel = rng.random(flat.size) < 0.04
    flat[sel] = SPECIAL[rng.integers(0, len(SPECIAL), int(sel.sum()))]
    zero = np.flatnonzero(flat == 0)
    flat[zero[rng.random(zero.size) < 0.5]] = -0.0
    with np.errstate(over="ignore"):
        return v.astype(dt)


def _np(a):
    if hasattr(a, "detach"):
        return a.detach().cpu().numpy()
    if hasattr(a, "to_numpy"):
        return a.to_numpy()
    return np.asarray(a)


def _bits_equal(got, want, what):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64), err_msg=what)


def assert_first_holder(samples, values, edges, axis, amin, amax, vmin, vmax):
    """the property, without the oracle's sort: for every non-empty bin the value at argmin has the key of vmin, and no counted
    sample before it has that key (the same for the maximum)"""
    arrays = np.broadcast_arrays(*samples, values)
    axis = normalise_axis(axis, arrays[0].ndim)
    rows = [ao.rows_cols_sorted(a, axis) for a in arrays]
    v = rows[-1].astype(F64)
    m, c = v.shape
    ok, flat, nbs = ao.counted_bins(rows[:-1], edges, v)
    nb = int(np.prod(nbs))
    k = eo.key(v)
    r = np.broadcast_to(np.arange(m)[:, None], (m, c))
    pos = np.broadcast_to(np.arange(c), (m, c))
    for at, ext in ((amin, vmin), (amax, vmax)):
        at, ext = np.asarray(at).reshape(m, nb), np.asarray(ext, F64).reshape(m, nb)
        filled = at >= 0
        np.testing.assert_array_equal(filled, ~np.isnan(ext))
        hist = np.bincount((r * nb + flat)[ok], minlength=m * nb).reshape(m, nb)
        np.testing.assert_array_equal(filled, hist > 0)
        assert (at < c).all()
        rr, bb = np.nonzero(filled)
        np.testing.assert_array_equal(k[rr, at[rr, bb]], eo.key(ext[rr, bb]))  # the holder holds the extreme
        assert ok[rr, at[rr, bb]].all() and (flat[rr, at[rr, bb]] == bb).all()  # ... is counted, and in this bin
        same = ok & (k == eo.key(np.where(np.isnan(ext), 0.0, ext))[r, flat]) & filled[r, flat]
        assert not (same & (pos < at[r, flat])).any(), "a counted sample before the reported one holds the extreme"


def check(core, args, values, bins, axis=None, host=None, want_desc=None, what=""):
    """args / values as handed to the call; host: their numpy images (samples, values) where they are device views of
    something else.  Returns (argmin, argmax, vmin, vmax) as numpy arrays and the parsed describe() line."""
    amin, amax, vmin, vmax, edges = core.histogram_argextrema(*args, values=values, bins=bins, axis=axis)
    got_desc = None
    if want_desc is not None:
        torch.cuda.synchronize()
        got_desc = assert_variant(_plan_for(core, args, edges).describe(), want_desc)
    emin, emax, _ = core.histogram_extrema(*args, values=values, bins=bins, axis=axis)
    for a in (amin, amax):
        assert (a.dtype == torch.int64) if hasattr(a, "detach") else (a.dtype == np.int64)
    if hasattr(values, "detach"):
        assert amin.is_cuda and vmin.is_cuda and vmin.dtype == torch.float64
    hs, hv = host if host is not None else ([_np(a) for a in args], _np(values))
    edges = [_np(e) for e in edges]
    want = ao.histogram_argextrema(*hs, values=hv, bins=edges, axis=axis)
    got = [_np(a) for a in (amin, amax, vmin, vmax)]
    np.testing.assert_array_equal(got[0], want[0], err_msg="argmin " + what)
    np.testing.assert_array_equal(got[1], want[1], err_msg="argmax " + what)
    _bits_equal(got[2], want[2], "vmin " + what)
    _bits_equal(got[3], want[3], "vmax " + what)
    _bits_equal(got[2], _np(emin), "vmin against histogram_extrema " + what)
    _bits_equal(got[3], _np(emax), "vmax against histogram_extrema " + what)
    assert_first_holder(hs, hv, edges, axis, *got)
    return got, got_desc


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1. census: the fast family's twelve kernels
# ---------------------------------------------------------------------------------------------------------------------
# form -> (edge kind, bins for D = 1 per sample type, bins per input for D = 2 per sample type), fine, arith
FAST_FORMS = {
    "scan1": ("k1", {F64: (300,), F32: (300,)}, {F64: (24, 30), F32: (24, 30)}, 1, False),
    "scan2": ("k2", {F64: (300,), F32: (300,)}, {F64: (24, 30), F32: (24, 30)}, 2, False),
    # np.linspace edges whose fine tables no longer fit next to the 32- / 24-byte slots: the table-free digitize
    "arith": ("lin", {F64: (5_000,), F32: (6_500,)}, {F64: (3, 1_600), F32: (3, 2_100)}, 1, True),
}


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("sdt", ["f64", "f32"])
@pytest.mark.parametrize("form", list(FAST_FORMS))
def test_fast_kernels(xh, form, sdt, D):
    kind, nb1, nb2, fine, arith = FAST_FORMS[form]
    st = F64 if sdt == "f64" else F32
    seed = 500 + 10 * list(FAST_FORMS).index(form) + 2 * D + (st == F32)
    edges = [edges_of(kind, nb, seed=seed + d) for d, nb in enumerate((nb1 if D == 1 else nb2)[st])]
    n_rows, n_cols = 3, 20_011
    want = predict(_cus(), edges, 0, st, st, n_rows, n_cols, fine, arith)
    assert want["family"] == "fast" and want["scan"] == {"scan1": 1, "scan2": 2, "arith": 5}[form], want
    xs = float_samples(edges, n_rows, n_cols, st, seed)
    v = tie_values(np.random.default_rng(seed), xs[0].shape, st)
    check(xh, [dev(x) for x in xs], dev(v), edges, axis=1, want_desc=want, what="%s %s D=%d" % (form, sdt, D))


def test_each_pass_has_its_own_residency(xh):
    """5 000 bins of 16 bytes leave room for two of pass 1's workgroups on a CU, 32 bytes for one of pass 2's: a row long
    enough for both gets twice the segments in pass 1"""
    edges = [edges_of("lin", 5_000, seed=3)]
    n_cols = 2048 * 600 + 3
    want = predict(_cus(), edges, 0, F64, F64, 1, n_cols, 1, True)
    assert want["scan"] == 5 and want["segs"] == [min(601, 2 * _cus()), min(601, _cus())] and want["segs"][0] > want["segs"][1]
    xs = float_samples(edges, 1, n_cols, F64, 3)
    v = tie_values(np.random.default_rng(3), xs[0].shape, F64)
    check(xh, [dev(x) for x in xs], dev(v), edges, axis=1, want_desc=want, what="two residencies")


# ---------------------------------------------------------------------------------------------------------------------
# 2. census: the generic family's six kernels, and both places its tables are read from
# ---------------------------------------------------------------------------------------------------------------------
HOME_BINS = {"lds": 200, "global": 9_000, "global_tables_l2": 21_000}


@pytest.mark.parametrize("home", list(HOME_BINS))
@pytest.mark.parametrize("dom", ["f64", "i64", "mixed"])
def test_generic_kernels(xh, dom, home):
    rng = np.random.default_rng(60 + 3 * ["f64", "i64", "mixed"].index(dom) + list(HOME_BINS).index(home))
    nb = HOME_BINS[home] if dom != "mixed" else max(2, HOME_BINS[home] // 6)
    if dom == "mixed" and home == "global_tables_l2":
        nb = 21_000  # (the int64 input's edges alone must leave LDS)
    edges = _domain_edges(dom, nb, rng)
    n_rows, n_cols = 2, 20_011
    cmp = {"f64": 0, "i64": 1, "mixed": 3}[dom]
    xs = []
    for d, e in enumerate(edges):
        xs += float_samples([e], n_rows, n_cols, F64, 7 + d) if np.asarray(e).dtype.kind == "f" else int_samples([e], n_rows, n_cols, None, 7 + d)
    v = tie_values(rng, (n_rows, n_cols), {"f64": F32, "i64": np.int32, "mixed": F64}[dom])  # (f64: another type than the samples)
    want = predict(_cus(), edges, cmp, xs[0].dtype, v.dtype, n_rows, n_cols, fine=False)
    assert want["family"] == "generic" and want["slots"] == ("lds" if home == "lds" else "global")
    assert want["tables_in_lds"] == (0 if home == "global_tables_l2" else 1)
    check(xh, [dev(x) for x in xs], dev(v), edges, axis=1, want_desc=want, what="%s %s" % (dom, home))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the LDS borders of the 32-byte (24-byte) slot: the last bin count a family or home takes, and the next one
# ---------------------------------------------------------------------------------------------------------------------
def border_cases():
    """(border, sample dtype, bins, edge kind) for both sides of every border of the pass-2 slot"""
    out = []
    n = _last(lambda n: table_bytes([np.zeros(n + 1)], "native") + n * 32 <= LDS_MAX)
    out += [("generic_lds", "gen", n, "k1"), ("generic_lds", "gen", n + 1, "k1")]
    for st, slot, fine_t in ((F64, 32, "fine64"), (F32, 24, "fine32")):
        n = _last(lambda n: table_bytes([np.zeros(n + 1)], fine_t) + n * slot <= LDS_MAX)
        out += [("fine", st, n, "k1"), ("fine", st, n + 1, "k1"), ("fine", st, n + 1, "lin")]
        n = LDS_MAX // slot
        out += [("arith", st, n, "lin"), ("arith", st, n + 1, "lin")]
    return out


def _border_predict(i, n_cols=30_011, cus=256):
    border, sdt, nb, kind = BORDERS[i]
    st = F64 if sdt == "gen" else sdt
    vdt = F32 if sdt == "gen" else st  # (another value type: the generic family)
    edges = [edges_of(kind, nb, seed=700 + i)]
    return edges, st, vdt, predict(cus, edges, 0, st, vdt, 1, n_cols, True, kind == "lin")


BORDERS = border_cases()


def test_borders_sit_where_the_slots_say():
    sides, landed = {}, {}
    for i, (border, st, nb, kind) in enumerate(BORDERS):
        sides.setdefault((border, getattr(st, "__name__", st)), []).append(nb)
        w = _border_predict(i)[3]
        landed[(border, getattr(st, "__name__", st), nb, kind)] = (w["family"], w["slots"], w["scan"])
    assert sides[("arith", "float64")] == [5120, 5121]  # 160 KiB / 32 B
    assert sides[("arith", "float32")] == [6826, 6827]  # 160 KiB / 24 B
    n = sides[("generic_lds", "gen")][0]
    tb = table_bytes([np.zeros(n + 1)], "native")
    assert n == (LDS_MAX - tb) // 32 and sides[("generic_lds", "gen")][1] == n + 1
    assert landed[("generic_lds", "gen", n, "k1")][:2] == ("generic", "lds")
    assert landed[("generic_lds", "gen", n + 1, "k1")][:2] == ("generic", "global")
    # between the 16- and the 32-byte capacity histogram_extrema alone keeps its slots in LDS; histogram_argextrema does not
    assert table_bytes([np.zeros(n + 2)], "native") + (n + 1) * 16 <= LDS_MAX
    for sdt in ("float64", "float32"):
        a, b = sides[("arith", sdt)]
        assert landed[("arith", sdt, a, "lin")] == ("fast", "lds", 5) and landed[("arith", sdt, b, "lin")][0] == "generic"
        a, b = sides[("fine", sdt)][:2]
        assert landed[("fine", sdt, a, "k1")][:2] == ("fast", "lds") and landed[("fine", sdt, a, "k1")][2] != 5
        assert landed[("fine", sdt, b, "k1")][0] == "generic"  # no table, no arithmetic edges
        assert landed[("fine", sdt, b, "lin")] == ("fast", "lds", 5)  # arithmetic edges: table-free


@pytest.mark.parametrize("i", range(len(BORDERS)), ids=["%s-%s-%d-%s" % (b, getattr(t, "__name__", t), n, k) for b, t, n, k in BORDERS])
def test_lds_border(xh, i):
    border, sdt, nb, kind = BORDERS[i]
    n_cols = 30_011
    edges, st, vdt, _ = _border_predict(i)
    want = _border_predict(i, n_cols, _cus())[3]
    xs = float_samples(edges, 1, n_cols, st, 700 + i)
    v = tie_values(np.random.default_rng(700 + i), xs[0].shape, vdt)
    check(xh, [dev(x) for x in xs], dev(v), edges, axis=1, want_desc=want, what="border %s %d" % (border, nb))


# ---------------------------------------------------------------------------------------------------------------------
# 4. tile borders: where the true extreme sits, one row shared by several workgroups and a few rows
# ---------------------------------------------------------------------------------------------------------------------
TILES = {"fast_f64": (F64, F64, 2048), "fast_f32": (F32, F32, 4096), "fast_f64_pairs": (F64, F64, 2048), "generic": (F64, F32, 512)}


@pytest.mark.parametrize("cols", ["1", "tile-1", "tile", "tile+1", "3*tile+5"])
@pytest.mark.parametrize("family", list(TILES))
def test_tile_borders(xh, family, cols):
    st, vdt, tile = TILES[family]
    n_cols = {"1": 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3*tile+5": 3 * tile + 5}[cols]
    D = 2 if family.endswith("pairs") else 1
    edges = [np.array([0.0, 1.0, 2.0, 4.0])] * D
    rng = np.random.default_rng(n_cols + D)
    places = sorted({min(3, n_cols - 1), min(tile + 7, n_cols - 1), n_cols - 1})  # first tile, a middle tile, the ragged tail
    for n_rows in (1, 3):
        want = predict(_cus(), edges, 0, st, vdt, n_rows, n_cols)
        assert want["family"] == family.split("_")[0] and want["segs"] == [-(-n_cols // tile)] * 2, want
        for at in places:
            xs = [rng.uniform(0.0, 4.0, (n_rows, n_cols)).astype(st) for _ in range(D)]
            v = tie_values(rng, (n_rows, n_cols), vdt)
            v[np.abs(v) > 50] = 1.0
            # the row's extremes, once each, in bin 0 of every input
            lo, hi = (at, (at + 1) % n_cols) if n_cols > 1 else (0, 0)
            for x in xs:
                x[:, [lo, hi]] = 0.5
            v[:, lo], v[:, hi] = (-100.0, 100.0) if n_cols > 1 else (5.0, 5.0)
            got, _ = check(xh, [dev(x) for x in xs], dev(v), edges, axis=1, want_desc=want,
                           what="%s cols %d extreme at %d rows %d" % (family, n_cols, at, n_rows))
            first = (0,) * D
            assert (got[0][(slice(None),) + first] == lo).all() and (got[1][(slice(None),) + first] == hi).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. ties
# ---------------------------------------------------------------------------------------------------------------------
EDGES3 = np.array([0.0, 1.0, 2.0, 3.0])


@pytest.mark.parametrize("family", ["fast_f64", "fast_f32", "generic"])
def test_constant_values_give_each_bins_first_counted_position(xh, family):
    st, vdt, tile = TILES[family]
    n_cols = 5 * tile + 11
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.5, 3.5, (2, n_cols)).astype(st)
    x[:, :40] = np.nan  # the first counted position is no small one
    x[0, 40:2 * tile] = 0.5  # row 0: bins 1 and 2 first appear in later workgroups' tiles
    v = np.full((2, n_cols), 7, vdt)
    got, _ = check(xh, [dev(x)], dev(v), [EDGES3], axis=1, what="constant " + family)
    np.testing.assert_array_equal(got[0], got[1])
    for r in range(2):
        for b in range(3):
            assert got[0][r, b] == np.flatnonzero((x[r] >= b) & (x[r] < b + 1))[0]
    assert got[0][0, 1] >= 2 * tile


def test_boolean_values(xh):
    rng = np.random.default_rng(6)
    x = rng.uniform(-0.5, 3.5, (3, 9_001))
    v = rng.random((3, 9_001)) < 0.5
    v[2] = True  # a row without a False
    got, _ = check(xh, [dev(x)], dev(v), [EDGES3], axis=1, what="bool")
    np.testing.assert_array_equal(got[0][2], got[1][2])
    check(xh, [x], v, [EDGES3], axis=1, what="bool numpy")


def test_values_broadcast_along_a_reduced_axis(xh):
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.5, 3.5, (4, 50, 60))
    for shape in ((4, 1, 60), (1, 50, 1), (4, 1, 1)):  # stride 0 along axis 1, along axes 0 and 2, along both reduced axes
        v = tie_values(rng, shape, F64)
        check(xh, [dev(x)], dev(v), [EDGES3], axis=(1, 2), what="broadcast %s" % (shape,))
        check(xh, [x], v, [EDGES3], axis=(1, 2), what="broadcast numpy %s" % (shape,))


@pytest.mark.parametrize("family", ["fast_f64", "fast_f32", "generic"])
def test_the_same_extreme_in_two_workgroups_tiles(xh, family):
    st, vdt, tile = TILES[family]
    n_cols = 4 * tile
    rng = np.random.default_rng(8)
    x = rng.uniform(0.0, 1.0, (1, n_cols)).astype(st)
    v = rng.integers(-3, 4, (1, n_cols)).astype(vdt)
    v[0, [9, 2 * tile + 5]] = -50  # tiles 0 and 2
    v[0, [tile + 3, 3 * tile + 1]] = 50  # tiles 1 and 3
    want = predict(_cus(), [EDGES3], 0, st, vdt, 1, n_cols)
    assert want["segs"] == [4, 4]
    got, _ = check(xh, [dev(x)], dev(v), [EDGES3], axis=1, want_desc=want, what="two tiles " + family)
    assert got[0][0, 0] == 9 and got[1][0, 0] == tile + 3


@pytest.mark.parametrize("dt", [F64, F32])
def test_uncounted_holders_before_the_first_counted_one(xh, dt):
    """NaN values, and out-of-range and NaN samples that carry the extreme value, at positions before the true first"""
    n = 5_000
    x = np.full(n, 0.5, dt)
    v = np.zeros(n, dt)
    v[[100, 200, 300, 4_000]] = -9.0
    v[[150, 250, 350, 4_500]] = 9.0
    x[[100, 150]] = 7.0  # out of range
    x[[200, 250]] = np.nan  # NaN samples
    v[:50] = np.nan  # NaN values in front
    got, _ = check(xh, [dev(x)], dev(v), [EDGES3], what="uncounted holders")
    assert got[0][0] == 300 and got[1][0] == 350
    assert got[0][1] == -1 and got[1][2] == -1 and np.isnan(got[2][1])


@pytest.mark.parametrize("dt", [F64, F32])
def test_signed_zeros_and_special_values(xh, dt):
    x = np.full(8, 0.5, dt)
    v = np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, np.nan, 0.0], dt)
    got, _ = check(xh, [dev(x)], dev(v), [EDGES3], what="zeros")
    assert got[0][0] == 2 and got[1][0] == 0  # argmin the first -0.0, argmax the first +0.0
    assert np.signbit(got[2][0]) and not np.signbit(got[3][0])
    # every special value of test_gpu_extrema.SPECIAL, twice each, one bin per pair of neighbours in the total order
    with np.errstate(over="ignore"):
        s = SPECIAL.astype(dt)
    s = s[~np.isnan(s)]
    vals = np.concatenate([s, s, s[::-1]])
    xs = np.concatenate([np.arange(len(s)), np.arange(len(s)), np.arange(len(s))[::-1]]).astype(dt) // 2 + 0.5
    check(xh, [dev(xs)], dev(vals), [np.arange(0.0, len(s) // 2 + 2)], what="special")
    check(xh, [dev(np.full(len(vals), 0.5, dt))], dev(vals), [EDGES3], what="special, one bin")


# ---------------------------------------------------------------------------------------------------------------------
# 6. layouts and backends
# ---------------------------------------------------------------------------------------------------------------------
def test_axis_orders_and_non_adjacent_axes(xh):
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.5, 3.5, (6, 50, 40))
    v = tie_values(rng, x.shape, F64)
    ref = None
    for axis in ((0, 2), (2, 0), (-1, 0)):  # unsorted and negative spellings of the same, non-adjacent, reduced axes
        for args, val in (([dev(x)], dev(v)), ([x], v)):
            got, _ = check(xh, args, val, [EDGES3], axis=axis, what="axis %s" % (axis,))
            ref = ref or got
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b)
    i0, i2 = np.unravel_index(np.maximum(ref[0], 0), (6, 40))  # C order over (axis 0, axis 2)
    j = np.broadcast_to(np.arange(50)[:, None], ref[0].shape)
    _bits_equal(np.where(ref[0] >= 0, v[i0, j, i2], np.nan), ref[2], "unravelled positions")
    for axis in (None, (1, 2), (2, 1), (2,), (0,), (1,), (0, 1, 2), (2, 0, 1)):  # (1,): grouped rows
        check(xh, [dev(x)], dev(v), [EDGES3], axis=axis, what="axis %s" % (axis,))
        check(xh, [x], v, [EDGES3], axis=axis, what="axis %s numpy" % (axis,))


def test_fortran_order_keeps_c_order_positions(xh):
    rng = np.random.default_rng(10)
    x = rng.uniform(-0.5, 3.5, (70, 90))
    v = tie_values(rng, x.shape, F64)
    xt, vt = dev(x.T).T, dev(v.T).T  # Fortran-ordered device tensors of the same logical arrays
    assert xt.stride() == (1, 70) and not xt.is_contiguous()
    a, _ = check(xh, [xt], vt, [EDGES3], host=([x], v), what="fortran torch")
    b, _ = check(xh, [np.asfortranarray(x)], np.asfortranarray(v), [EDGES3], what="fortran numpy")
    c, _ = check(xh, [dev(x)], dev(v), [EDGES3], what="c order")
    for p, q, r in zip(a, b, c):
        np.testing.assert_array_equal(p, r)
        np.testing.assert_array_equal(q, r)
    # a transposed 3-D view reduced over its first two axes
    x3 = rng.uniform(-0.5, 3.5, (5, 30, 20))
    v3 = tie_values(rng, x3.shape, F64)
    check(xh, [dev(x3).permute(1, 0, 2)], dev(v3).permute(1, 0, 2), [EDGES3], axis=(0, 1),
          host=([x3.transpose(1, 0, 2)], v3.transpose(1, 0, 2)), what="permuted")


@pytest.mark.parametrize("dt", [F64, F32])
def test_unaligned_row_starts(xh, dt):
    rng = np.random.default_rng(11)
    x = rng.uniform(-0.5, 3.5, (4, 10_000)).astype(dt)
    v = tie_values(rng, x.shape, dt)
    xd, vd = dev(x)[:, 1:], dev(v)[:, 1:]  # odd row lengths, the data one element in: not 16-byte aligned
    assert xd.data_ptr() % 16 and vd.data_ptr() % 16
    want = predict(_cus(), [EDGES3], 0, dt, dt, 4, 9_999)
    assert want["family"] == "fast"
    check(xh, [xd], vd, [EDGES3], axis=1, host=([x[:, 1:]], v[:, 1:]), want_desc=want, what="unaligned")


def test_backends(xh):
    from xhistogram_amd.devicearray import DeviceArray

    rng = np.random.default_rng(12)
    x = rng.uniform(-0.5, 3.5, (4, 30_000))
    v = tie_values(rng, x.shape, F64)
    amin, amax, vmin, vmax, edges = xh.histogram_argextrema(x, values=v, bins=[EDGES3], axis=1, block_size=64)
    assert all(isinstance(a, np.ndarray) for a in (amin, amax, vmin, vmax))
    assert amin.dtype == amax.dtype == np.int64 and vmin.dtype == vmax.dtype == np.float64 and amin.shape == vmin.shape == (4, 3)
    a, _ = check(xh, [x], v, [EDGES3], axis=1, what="numpy")
    b, _ = check(xh, [dev(x)], dev(v), [EDGES3], axis=1, what="torch")
    out = xh.histogram_argextrema(DeviceArray.from_numpy(x), values=DeviceArray.from_numpy(v), bins=[EDGES3], axis=1)
    assert all(isinstance(o, np.ndarray) for o in out[:4])
    for p, q, r in zip(a, b, out[:4]):
        np.testing.assert_array_equal(p, q)
        np.testing.assert_array_equal(p, r)
    # int bins: the edges of the unweighted histogram
    _, _, _, _, e = xh.histogram_argextrema(x, values=v, bins=50)
    np.testing.assert_array_equal(e[0], xh.histogram(x, bins=50)[1][0])


def test_empty_input_and_empty_bins(xh):
    for args, val in (([np.zeros(0)], np.zeros(0)), ([torch.zeros(0, dtype=torch.float64, device="cuda")], torch.zeros(0, dtype=torch.float64, device="cuda"))):
        amin, amax, vmin, vmax, _ = xh.histogram_argextrema(*args, values=val, bins=[EDGES3])
        amin, amax, vmin, vmax = (_np(a) for a in (amin, amax, vmin, vmax))
        assert amin.shape == (3,) and amin.dtype == np.int64 and (amin == -1).all() and (amax == -1).all()
        assert np.isnan(vmin).all() and np.isnan(vmax).all()
    amin, _, vmin, _, _ = xh.histogram_argextrema(np.zeros((0, 5)), values=np.zeros((0, 5)), bins=[EDGES3], axis=1)
    assert amin.shape == vmin.shape == (0, 3)
    amin, _, vmin, _, _ = xh.histogram_argextrema(np.zeros((4, 0)), values=np.zeros((4, 0)), bins=[EDGES3], axis=1)
    assert amin.shape == (4, 3) and (amin == -1).all() and np.isnan(vmin).all()
    # every bin empty: samples outside the range, NaN samples, NaN values
    x = np.r_[np.full(3_000, 9.0), np.full(3_000, np.nan), np.full(3_000, 0.5)]
    v = np.r_[np.ones(6_000), np.full(3_000, np.nan)]
    for dt in (F64, F32):
        got, _ = check(xh, [dev(x.astype(dt))], dev(v.astype(dt)), [EDGES3], what="every bin empty")
        assert (got[0] == -1).all() and (got[1] == -1).all() and np.isnan(got[2]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7. positions beyond 2^32
# ---------------------------------------------------------------------------------------------------------------------
def test_positions_beyond_32_bits(xh):
    """more than 2^32 columns in one row: one float64 sample broadcast with stride 0, uint8 ones as values with a 0 at
    2^32 + 7 and a 2 at 2^32 + 9 (4.3 GB; the generic family, one bin).  A 32-bit position would give 7 and 9."""
    n = (1 << 32) + 4096
    free, _ = torch.cuda.mem_get_info()
    assert free > n + (2 << 30), "needs %.1f GB of free device memory, %.1f GB free" % (n / 1e9, free / 1e9)
    v = torch.ones(n, dtype=torch.uint8, device="cuda")
    v[(1 << 32) + 7] = 0
    v[(1 << 32) + 9] = 2
    x = torch.full((1,), 0.5, dtype=torch.float64, device="cuda").expand(n)
    assert x.stride() == (0,)
    edges = [np.array([0.0, 1.0])]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    amin, amax, vmin, vmax, _ = xh.histogram_argextrema(x, values=v, bins=edges)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    desc = _plan_for(xh, [x], edges).describe()
    print("\n2^32 + 4096 columns: %.2f s; %s" % (dt, desc))
    got = parse(desc)
    assert got["family"] == "generic" and got["slots"] == "lds" and min(got["segs"]) >= 3
    assert int(amin[0]) == (1 << 32) + 7 and int(amax[0]) == (1 << 32) + 9
    assert float(vmin[0]) == 0.0 and float(vmax[0]) == 2.0
    del v
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# 8. dask, in the interpreter that has it
# ---------------------------------------------------------------------------------------------------------------------
PY39 = "/opt/conda/bin/python3.9"
SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "argextrema_dask_script.py")


def _have_dask_python():
    return os.path.exists(PY39) and subprocess.run([PY39, "-c", "import dask.array, numpy"], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_dask_python(), reason="no interpreter with dask in this image")
def test_dask_blocks_complete_along_the_reduced_axes():
    env = dict(os.environ)
    sys_cxx = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"  # (as tests/test_dask_branch.py: conda's libstdc++ is older)
    if os.path.exists(sys_cxx):
        env["LD_PRELOAD"] = (sys_cxx + ":" + env["LD_PRELOAD"]) if env.get("LD_PRELOAD") else sys_cxx
    r = subprocess.run([PY39, "-W", "ignore", SCRIPT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ARGEXTREMA-DASK-OK" in r.stdout
