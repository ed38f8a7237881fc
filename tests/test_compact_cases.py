"""CPU side of the class-map tests of the compaction ("Class-map tests of the compaction"):
the reference of tests/compact_cases.py against a plain loop and against the renderer (the CPU
oracle's frames), and the edges the GPU families are there for, asserted from numpy alone."""
import ctypes

import numpy as np
import pytest

import compact_cases as cc
from helpers import oracle_lib, rc

I64 = np.int64


# ---------------------------------------------------------- the reference is the definition --
def _same_lists(ref, cls):
    dep, ss, sk = cc.segment_slow(cls)
    return (np.array_equal(ref.dep, dep) and np.array_equal(ref.seg_start, ss) and np.array_equal(ref.seg_key, sk)
            and ref.ndep == len(dep) and ref.nseg == len(ss))


def test_segment_ref_is_the_sequential_scan():
    """Every map of up to 6 pixels in every shape, and seeded maps, against the loop over the pixels;
    the batched form against the single one."""
    n = 0
    for W, H in cc.small_shapes(6):
        maps = cc.small_batch(W, H)
        batch = cc.segment_ref(maps)
        dep, ss, sk = cc.padded_tables(batch, W * H + 1, -5, -5)
        for b, m in enumerate(maps):
            one = cc.segment_ref(m)
            assert _same_lists(one, m), (W, H, m)
            assert np.array_equal(dep[b, :one.ndep], one.dep) and (dep[b, one.ndep:] == -5).all()
            assert np.array_equal(ss[b, :one.nseg], one.seg_start) and (ss[b, one.nseg:] == -5).all()
            assert np.array_equal(sk[b, :one.nseg], one.seg_key) and (sk[b, one.nseg:] == -5).all()
            for k in ("rows", "row_off", "row_soff", "row_prevw", "row_prevd"):
                assert np.array_equal(getattr(batch, k)[b], getattr(one, k)), (k, m)
            n += 1
    assert n == sum(3 ** (W * H) for W, H in cc.small_shapes(6))
    for c in cc.density_cases()[:6] + cc.straddle_cases(8)[:2] + cc.rows_cases()[:20]:
        assert _same_lists(c.ref, c.cls), c


def test_row_tables_are_the_sequential_scan():
    """RowStats and the four per-row prefixes against a loop over the rows."""
    for c in cc.density_cases()[:9] + cc.straddle_cases(64)[:1] + cc.rows_cases()[:24]:
        m, r = c.cls, c.ref
        H, W = m.shape
        ndep = nseg = 0
        lastw = lastd = -1
        for y in range(H):
            assert (r.row_off[y], r.row_soff[y], r.row_prevw[y], r.row_prevd[y]) == (ndep, nseg, lastw, lastd), (c, y)
            row = m[y]
            dx, wx = np.flatnonzero(row == cc.DEP), np.flatnonzero(row == cc.WRITER)
            st = r.rows[y]
            assert st["ndep"] == len(dx)
            assert st["lastw"] == (y * W + wx[-1] if len(wx) else -1)
            assert st["lastd"] == (y * W + dx[-1] if len(dx) else -1)
            before = wx[wx < dx[0]] if len(dx) else wx[:0]
            assert st["wfirst"] == (y * W + before[-1] if len(before) else -1)
            inside = sum(1 for a, b in zip(dx[:-1], dx[1:]) if ((wx > a) & (wx < b)).any())
            assert st["nstart"] == inside, (c, y)
            starts = r.seg_start[(r.dep[r.seg_start] // W) == y]
            ndep += len(dx)
            nseg += len(starts)
            lastw = max(lastw, st["lastw"])
            lastd = max(lastd, st["lastd"])
        assert (ndep, nseg) == (r.ndep, r.nseg)


def _carry_outs(scene, W, H, pix):
    lib = oracle_lib()
    lib.rco_pixels.argtypes = [ctypes.POINTER(rc.JsonDataT)] + [ctypes.c_int] * 4 + [ctypes.c_int64] + [ctypes.c_void_p] * 6
    pix = np.ascontiguousarray(pix, I64)
    n = len(pix)
    rgb, cout = np.zeros((n, 3), np.uint8), np.zeros((n, 3), np.float32)
    cls, z = np.zeros(n, np.uint8), np.zeros(n, I64)
    assert lib.rco_pixels(ctypes.byref(scene.js), W, H, cc.NATURAL_DEPTH + 1, rc.MODES["parity"], n, pix.ctypes.data, None,
                          rgb.ctypes.data, cout.ctypes.data, cls.ctypes.data, z.ctypes.data) == 0
    return cout, cls


@pytest.mark.parametrize("name,W,H", cc.NATURAL, ids=[f"{n}-{W}x{H}" for n, W, H in cc.NATURAL])
def test_segment_ref_is_the_renderers(name, W, H):
    """On the oracle's class map: the carry-in that rco_render_cls reports at each segment's first
    entry is, bit for bit, rco_pixels' carry-out of the pixel seg_key names, or +0 without a key."""
    scene, cls, cin = cc.natural_frame(name, W, H)
    r = cc.segment_ref(cls)
    first = r.dep[r.seg_start]
    want = np.zeros((r.nseg, 3), np.float32)
    keyed = r.seg_key >= 0
    cout, kcls = _carry_outs(scene, W, H, r.seg_key[keyed])
    assert (kcls == cc.WRITER).all()
    want[keyed] = cout
    assert np.array_equal(cin[first].view(np.uint32), want.view(np.uint32)), (name, W, H)
    print(f"[compact_cases] {name} {W}x{H}: {r.ndep} DEP pixels, {r.nseg} segments, {int(keyed.sum())} keyed")


# ------------------------------------------------------------------------------ the edges --
def test_natural_frames_cross_both_chunks():
    _, cls, _ = cc.natural_frame("reflection", 8195, 3)
    assert int((cls[:, cc.ROW_CHUNK:] == cc.DEP).sum()) == 770
    r = cc.segment_ref(cls)
    assert int(((r.dep[r.seg_start] % 8195) >= cc.ROW_CHUNK).sum()) == 1
    _, cls, _ = cc.natural_frame("reflection", 3, 4099)
    r = cc.segment_ref(cls)
    assert int((r.dep // 3 >= cc.SCAN_CHUNK).sum()) == 1129
    assert int((r.dep[r.seg_start] // 3 >= cc.SCAN_CHUNK).sum()) == 160


@pytest.mark.parametrize("b", cc.STRADDLE_B)
def test_straddle_edges(b):
    """Every pattern is there over both backgrounds at every width, and from b = 64 on each required
    edge at least once."""
    cases = cc.straddle_cases(b)
    assert sorted({c.cls.shape[1] for c in cases}) == [b + d for d in cc.STRADDLE_DW]
    total = {}
    for W in {c.cls.shape[1] for c in cases}:
        for bg in ("ident", "sparse"):
            sub = [c for c in cases if c.cls.shape[1] == W and f"/{bg}/" in c.label]
            assert sorted(np.concatenate([c.patterns for c in sub])) == list(range(729))
            assert all(c.cls.size <= 2.1e6 for c in sub)
            for c in sub:
                for k, x in enumerate(range(b - 3, b + 3)):
                    if x < W:
                        assert np.array_equal(c.cls[:, x], cc.PATTERNS[c.patterns, k])
    for c in cases:
        for k, v in cc.straddle_edges(c).items():
            total[k] = total.get(k, 0) + v
    print(f"[compact_cases] straddle b {b}: {total}")
    if b >= 64:
        assert all(v > 0 for v in total.values()), total


def _ends(row):
    dx, wx = np.flatnonzero(row == cc.DEP), np.flatnonzero(row == cc.WRITER)
    if len(wx) and (not len(dx) or wx[-1] > dx[-1]):
        return "writer-last"
    return "dep-last" if len(dx) else "neither"


def _begins(row):
    dx, wx = np.flatnonzero(row == cc.DEP), np.flatnonzero(row == cc.WRITER)
    if not len(dx):
        return "no-dep"
    return "writer-dep" if len(wx) and wx[0] < dx[0] else "dep-first"


def test_rows_edges():
    cases = cc.rows_cases()
    shapes = {(c.cls.shape[1], c.cls.shape[0]) for c in cases if c.label.count("/") == 1}
    assert shapes == {(W, H) for W in cc.ROWS_W for H in cc.ROWS_H}
    for k in (2048, 4096):
        assert k % cc.SCAN_CHUNK == 0
        seen = {(_ends(c.cls[k - 1]), _begins(c.cls[k])) for c in cases if getattr(c, "boundary", 0) == k}
        assert seen == {(u, l) for u in cc.UPPER for l in cc.LOWER}, seen
        for c in cases:
            if getattr(c, "boundary", 0) == k:
                assert (_ends(c.cls[k - 1]), _begins(c.cls[k])) == c.combo
        st = {c.stretch[1] for c in cases if getattr(c, "stretch", (0, 0))[0] == k
              and (c.cls[k - 4:k + 4] == c.stretch[1]).all()}
        assert st == {cc.IDENT, cc.WRITER, cc.DEP}
    # a row of writers only before a scan-chunk boundary, a DEP pixel first after it
    assert {c.writers_only for c in cases if hasattr(c, "writers_only")} == {2048, 4096}
    for c in cases:
        if hasattr(c, "writers_only"):
            k = c.writers_only
            assert (c.cls[k - 1] == cc.WRITER).all() and c.cls[k, 0] == cc.DEP and (c.cls[:k - 1] == cc.DEP).any()


def test_density_and_many_edges():
    by = {c.label: c for c in cc.density_cases()}
    for W, H in cc.DENSITY_SHAPES:
        P = W * H
        r = by[f"density/{W}x{H}/all-ident"].ref
        assert (r.ndep, r.nseg) == (0, 0)
        r = by[f"density/{W}x{H}/all-writer"].ref
        assert (r.ndep, r.nseg) == (0, 0)
        r = by[f"density/{W}x{H}/all-dep"].ref
        assert (r.ndep, r.nseg) == (P, 1) and r.seg_key[0] == -1
        r = by[f"density/{W}x{H}/alternating"].ref
        assert r.ndep == r.nseg == P // 2
        r = by[f"density/{W}x{H}/dep-at-last"].ref
        assert (r.ndep, r.nseg, r.dep[0], r.seg_key[0]) == (1, 1, P - 1, -1)
        r = by[f"density/{W}x{H}/writer-first-dep-last"].ref
        assert (r.ndep, r.nseg, r.dep[0], r.seg_key[0]) == (1, 1, P - 1, 0)
    assert 4099 > cc.ROW_CHUNK
    assert [c.ref.nseg for c in cc.many_cases()] == [65792, 65535, 65536, 65537]
    assert cc.SEG_ORDER_MAX == 65536


def test_order_edges():
    cases = cc.order_cases()
    assert {len(ss) for _, ss, _, _, _ in cases} >= set(cc.ORDER_NSEG)
    assert {bm for _, _, _, bm, _ in cases} >= set(cc.ORDER_BLOCK_MIN)
    lens = set()
    for _, ss, ndep, _, _ in cases:
        lens |= set(np.diff(np.concatenate((ss.astype(I64), [ndep]))).tolist())
        assert ndep < 2 ** 31 and (np.diff(ss.astype(I64)) > 0).all()
    assert lens >= set(cc.ORDER_LENGTHS)
    # runs of equal buckets (stability shows), the long count at 2 * block_cap and one above
    assert any(lb.startswith("order/runs/n1000/") for lb, *_ in cases)
    hit = set()
    for lb, ss, ndep, bm, cap in cases:
        if lb.startswith("order/cap/"):
            ln = np.diff(np.concatenate((ss.astype(I64), [ndep])))
            n = int((np.minimum(ln >> 5, 255) >= min((bm + 31) // 32, 255)).sum())
            hit.add(n - 2 * cap)
            assert cc.order_ref(ss, ndep, bm, cap)[2] == (n if n <= 2 * cap else 0)
    assert hit == {0, 1}
    assert cc.order_ref(*cases[-1][1:])[0] is not None
    big = [c for c in cases if len(c[1]) == 65537]
    assert big and all(cc.order_ref(*c[1:]) == (None, 0, 0, 0) for c in big)


def test_shard_edges():
    cases = cc.shard_cases()
    assert {g for g, _ in cases} == set(cc.SHARD_G)
    for G in cc.SHARD_G:
        hs = {c.cls.shape[0] for g, c in cases if g == G}
        assert hs == set(cc.shard_heights(G))
        assert {c.cls.shape[1] for g, c in cases if g == G} == set(cc.SHARD_W)
        if G > 1:
            assert min(hs) < G      # ranks without a row
    # a rank whose rows hold no DEP pixel beside ranks that do (an empty list in the exchange)
    assert any(c.ref.ndep > 0 and any(not (c.cls[g::G] == cc.DEP).any() for g in range(min(G, c.cls.shape[0])))
               for G, c in cases if G > 1)
    assert {(3 * W) % 4 == 0 for _, W, _ in cc.DEINTERLEAVE} == {True, False}


def test_wkey_edges():
    """Every width from 1 to 17 and every density map are there; the whole-map form of the key-writer
    rule is test_layout.py's restatement on every map of the family; and each kind of map (density,
    straddle, the seeded widths) holds writers with either answer."""
    cases = cc.wkey_cases()
    assert {c.cls.shape[1] for c in cases} >= set(range(1, 18))
    assert all(c in cases for c in cc.density_cases()) and all(c in cases for c in cc.straddle_cases(8))
    both = {}
    for c in cases:
        assert np.array_equal(c.keep, cc.key_writers_loop(c.cls)), c
        w = c.cls == cc.WRITER
        kind = c.label.split("/")[0]
        s, n = both.get(kind, (False, False))
        both[kind] = (s or bool((c.keep & w).any()), n or bool((~c.keep & w).any()))
    assert both == {"density": (True, True), "straddle": (True, True), "wkey": (True, True)}, both
