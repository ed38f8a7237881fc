"""Progressive supersampling on the GPU (rc_accum_pass_device, rc_render_accum): after every pass
the accumulator and the image are the numpy contract's (rc.accum_step) on the CPU oracle's own
g*W x g*H image, byte for byte: no tolerance anywhere."""
import numpy as np
import pytest

from helpers import oracle_render, oracle_render_cuda, rc, scene_path

pytestmark = pytest.mark.gpu

SCENES = ["simple", "reflection", "quadric"]
SIZES = [(1, 1), (7, 3), (33, 17), (64, 48)]   # partial tiles, a one-wave image, a short list
CUDA_SIZES = [(7, 3), (64, 48)]
T = 16


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SCENES}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


_oracle = {}


def oracle_image(scenes, name, w, h, depth, mode):
    """The oracle's w x h image: computed once per key, read-only."""
    key = (name, w, h, depth, mode)
    if key not in _oracle:
        if mode == "cuda":
            img = oracle_render_cuda(scenes[name], w, h, depth)
        else:
            img, stats = oracle_render(scenes[name], w, h, depth, mode)
            assert stats["parity_defined"] == 1, key   # the example scenes are all defined
        img.setflags(write=False)
        _oracle[key] = img
    return _oracle[key]


def big_image(scenes, name, g, w, h, depth, mode):
    return oracle_image(scenes, name, g * w, g * h, depth, mode)


class State:
    """An accumulator and an image in device memory ([H, W, 4] int16 bits, [H, W, 3] uint8)."""

    def __init__(self, torch, w, h, acc=None, out=None, stream=None):
        self.torch, self.w, self.h = torch, w, h
        acc = np.zeros((h, w, 4), np.uint16) if acc is None else acc
        out = np.zeros((h, w, 3), np.uint8) if out is None else out
        assert acc.shape == (h, w, 4) and acc.dtype == np.uint16 and out.shape == (h, w, 3)
        self.stream = stream
        if stream is None:
            self.d_acc = torch.from_numpy(acc.view(np.int16).copy()).cuda()
            self.d_out = torch.from_numpy(out.copy()).cuda()
            torch.cuda.synchronize()
        else:   # uploaded on the stream the passes use, with no wait in between
            with torch.cuda.stream(stream):
                self.d_acc = torch.from_numpy(acc.view(np.int16).copy()).pin_memory().cuda(
                    non_blocking=True)
                self.d_out = torch.from_numpy(out.copy()).pin_memory().cuda(non_blocking=True)

    def run(self, scene, seq, first, count, t=0, reset=False, depth=6, mode="fast", timing=None):
        rc.accum_pass_device(scene, self.w, self.h, seq, first, count, self.d_acc.data_ptr(),
                             self.d_out.data_ptr(), threshold=t, reset=reset,
                             stream_ptr=self.stream.cuda_stream if self.stream else None,
                             depth=depth, mode=mode, timing=timing)

    def read(self):
        """(acc, out) as numpy arrays, after everything enqueued."""
        self.torch.cuda.synchronize()
        return self.d_acc.cpu().numpy().view(np.uint16), self.d_out.cpu().numpy()


def check_state(st, acc, out, tag):
    got_acc, got_out = st.read()
    np.testing.assert_array_equal(got_acc, acc, err_msg=f"acc {tag}")
    np.testing.assert_array_equal(got_out, out, err_msg=f"out {tag}")


def random_state(rng, h, w, nmax):
    """A valid accumulator: n in 0..nmax, each sum in 0..255 * n."""
    n = rng.integers(0, nmax + 1, size=(h, w), dtype=np.int64)
    acc = np.zeros((h, w, 4), dtype=np.uint16)
    acc[:, :, :3] = (rng.random((h, w, 3)) * (255 * n[:, :, None] + 1)).astype(np.int64).clip(
        0, 255 * n[:, :, None])
    acc[:, :, 3] = n
    return acc


def check_prefixes(torch, scenes, name, seqname, k, w, h, depth, mode):
    """A reset pass with sample 0, then one-sample t = 0 passes up to seq[0..k): after every pass
    d_acc and d_out are the contract's."""
    g, pts = rc.SAMPLE_SEQS[seqname]
    big = big_image(scenes, name, g, w, h, depth, mode)
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    st = State(torch, w, h, out=np.full((h, w, 3), 77, np.uint8))   # reset does not read it
    for j in range(k):
        acc, out, active, sat = rc.accum_step(acc, out, big, g, pts[j:j + 1], 0, reset=j == 0)
        st.run(scenes[name], seqname, j, 1, reset=j == 0, depth=depth, mode=mode)
        tag = f"{name} {seqname}[0..{j + 1}) {w}x{h} d{depth} {mode}"
        check_state(st, acc, out, tag)
        assert rc.accum_stats() == {"passes": 1, "active_pixels": w * h, "saturated": 0,
                                    "rays": w * h}, tag
    assert (acc[:, :, 3] == k).all()


@pytest.mark.parametrize("depth", [0, 6])
@pytest.mark.parametrize("scene", SCENES)
def test_prefixes_fast_vs_oracle(scene, depth, scenes, torch):
    for w, h in SIZES:
        check_prefixes(torch, scenes, scene, "hier8", 11, w, h, depth, "fast")   # 3, 5, 7, 11
        check_prefixes(torch, scenes, scene, "queens8", 8, w, h, depth, "fast")


@pytest.mark.parametrize("scene", SCENES)
def test_prefixes_cuda_vs_oracle(scene, scenes, torch):
    for w, h in CUDA_SIZES:
        check_prefixes(torch, scenes, scene, "hier8", 11, w, h, 50, "cuda")
        check_prefixes(torch, scenes, scene, "queens8", 8, w, h, 50, "cuda")


def run_split(torch, scene, seqname, split, w, h, mode="fast", depth=6, timings=None):
    """The passes of `split` (sample counts, the first resetting) at t = 0; the final state."""
    st = State(torch, w, h)
    first = 0
    for j, count in enumerate(split):
        tim = {} if timings is not None else None
        st.run(scene, seqname, first, count, reset=j == 0, depth=depth, mode=mode, timing=tim)
        if timings is not None:
            timings.append(tim)
        first += count
    return st.read()


def test_split_independence(scenes, torch):
    """On the GPU alone: a prefix in one call or in any split gives one state."""
    for name in SCENES:
        for w, h in SIZES:
            for mode, depth in (("fast", 6), ("cuda", 50)):
                if mode == "cuda" and (w, h) not in CUDA_SIZES:
                    continue
                one = run_split(torch, scenes[name], "hier8", [4], w, h, mode, depth)
                assert (one[0][:, :, 3] == 4).all()
                for split in ([1, 3], [2, 2], [1, 1, 1, 1]):
                    got = run_split(torch, scenes[name], "hier8", split, w, h, mode, depth)
                    tag = f"{name} {w}x{h} {mode} {split}"
                    np.testing.assert_array_equal(got[0], one[0], err_msg=tag)
                    np.testing.assert_array_equal(got[1], one[1], err_msg=tag)
    # the largest count against the smallest, and an odd one across the chunks
    sc = scenes["quadric"]
    one = run_split(torch, sc, "hier8", [16], 33, 17)
    for split in ([1] * 16, [5, 11], [15, 1]):
        got = run_split(torch, sc, "hier8", split, 33, 17)
        np.testing.assert_array_equal(got[0], one[0], err_msg=str(split))
        np.testing.assert_array_equal(got[1], one[1], err_msg=str(split))


@pytest.mark.parametrize("scene", SCENES)
def test_family_equalities(scene, scenes, torch):
    """On the GPU alone: a pattern's n samples are rc_render_pattern's bytes; the whole lattice of
    hier<g> is rc_options.ssaa = g, bytes and zero-normalize events."""
    sc = scenes[scene]
    for w, h in SIZES:
        for pat, (g, pts) in rc.PATTERNS.items():
            want = rc.render_pattern(sc, w, h, pat, depth=6, mode="fast")
            acc, out = run_split(torch, sc, pat, [len(pts)], w, h)
            np.testing.assert_array_equal(out, want, err_msg=f"{scene} {pat} {w}x{h}")
        for g in (2, 4, 8):
            ts, tims = {}, []
            want = rc.render(sc, w, h, depth=6, mode="fast", ssaa=g, timing=ts)
            split = [g * g] if g < 8 else [16, 16, 16, 16]
            acc, out = run_split(torch, sc, f"hier{g}", split, w, h, timings=tims)
            tag = f"{scene} hier{g} {w}x{h}"
            np.testing.assert_array_equal(out, want, err_msg=tag)
            assert (acc[:, :, 3] == g * g).all(), tag
            assert sum(t["zero_normalize"] for t in tims) == ts["zero_normalize"], tag
            assert all(t["kernel_ms"] > 0.0 for t in tims), tag
    want = rc.render(sc, 64, 48, depth=50, mode="cuda", ssaa=4)
    acc, out = run_split(torch, sc, "hier4", [16], 64, 48, "cuda", 50)
    np.testing.assert_array_equal(out, want)
    want = rc.render_pattern(sc, 7, 3, "queens8", depth=50, mode="cuda")
    acc, out = run_split(torch, sc, "queens8", [3, 5], 7, 3, "cuda", 50)
    np.testing.assert_array_equal(out, want)


def masked_chain(scenes, name, seqname, w, h, depth, mode):
    """The contract's states of one dense sample and then one-sample passes at T over the rest of
    the sequence, with what the test below needs to hold of them asserted on the CPU."""
    g, pts = rc.SAMPLE_SEQS[seqname]
    pts = pts[:8]   # hier8: its first eight points; rgss4 has four
    big = big_image(scenes, name, g, w, h, depth, mode)
    acc, out, _, _ = rc.accum_step(np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8),
                                   big, g, pts[:1], 0, reset=True)
    chain = [(acc, out, w * h, 0)]
    for j in range(1, len(pts)):
        acc, out, active, sat = rc.accum_step(acc, out, big, g, pts[j:j + 1], T)
        assert sat == 0
        chain.append((acc, out, active, sat))
    if (w, h) in ((33, 17), (64, 48)):
        key = (name, seqname, w, h, mode)
        assert all(0 < c[2] < w * h for c in chain[1:]), key   # neither empty nor everything
        assert (out != rc.accum_run(big, g, pts, len(pts), 0)).any(), key   # not the dense mean
        assert len(np.unique(acc[:, :, 3])) >= 3, key
    return chain


@pytest.mark.parametrize("mode,depth", [("fast", 6), ("cuda", 50)])
@pytest.mark.parametrize("scene", SCENES)
def test_masked_passes_vs_oracle(scene, mode, depth, scenes, torch):
    sizes = [(33, 17), (64, 48)] if mode == "fast" else [(64, 48)]
    chains = {(seq, w, h): masked_chain(scenes, scene, seq, w, h, depth, mode)
              for w, h in sizes for seq in ("hier8", "queens8", "rgss4")}
    for (seqname, w, h), chain in chains.items():   # nothing has touched the GPU so far
        st = State(torch, w, h)
        for j, (acc, out, active, sat) in enumerate(chain):
            tim = {}
            st.run(scenes[scene], seqname, j, 1, t=0 if j == 0 else T, reset=j == 0, depth=depth,
                   mode=mode, timing=tim)
            tag = f"{scene} {seqname} pass {j} {w}x{h} {mode}"
            check_state(st, acc, out, tag)
            assert rc.accum_stats() == {"passes": 1, "active_pixels": active, "saturated": 0,
                                        "rays": active}, tag
            ms = rc.accum_phase_ms()
            assert sorted(ms) == ["mark", "shoot"] and ms["shoot"] > 0.0, tag
            assert (ms["mark"] > 0.0) == (j > 0), tag
            assert ms["mark"] + ms["shoot"] == pytest.approx(tim["kernel_ms"], rel=1e-3), tag


def half_flat_image(rng, h, w):
    """An image the test chooses: noise on the left, one colour on the right, so that the edge
    mask at T is neither empty nor everything."""
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[:, w // 2:] = (90, 140, 200)
    return img


def test_inactive_pixels_keep_their_bytes(scenes, torch):
    """A prefilled image and a random valid state, uploaded on the stream the pass runs on: every
    pixel outside the edge mask of the image on entry keeps all 11 of its bytes; the others are
    the contract's."""
    rng = np.random.default_rng(21)
    stream = torch.cuda.Stream()
    for name, (w, h) in zip(SCENES, [(33, 17), (64, 48), (7, 3)]):
        g, pts = rc.SAMPLE_SEQS["queens8"]
        big = big_image(scenes, name, g, w, h, 6, "fast")
        out_in, acc_in = half_flat_image(rng, h, w), random_state(rng, h, w, 200)
        mask = rc.edge_mask(out_in, T)
        assert 0 < mask.sum() < w * h
        st = State(torch, w, h, acc_in, out_in, stream=stream)
        st.run(scenes[name], "queens8", 5, 1, t=T)
        got_acc, got_out = st.read()
        np.testing.assert_array_equal(got_acc[~mask], acc_in[~mask])
        np.testing.assert_array_equal(got_out[~mask], out_in[~mask])
        assert (got_acc[mask][:, 3] == acc_in[mask][:, 3] + 1).all()
        acc, out, active, sat = rc.accum_step(acc_in, out_in, big, g, pts[5:6], T)
        np.testing.assert_array_equal(got_acc, acc)
        np.testing.assert_array_equal(got_out, out)
        assert rc.accum_stats() == {"passes": 1, "active_pixels": int(mask.sum()), "saturated": 0,
                                    "rays": int(mask.sum())}


def test_resolve(torch):
    """1024 x 1024 records: every n in 0..256 with the smallest, the largest and random sums."""
    rng = np.random.default_rng(4)
    side = 1024
    acc = random_state(rng, side, side, 256)
    n = np.arange(257, dtype=np.uint16)
    acc[0, :257, 3], acc[0, :257, :3] = n, 0                          # sum = 0, n = 0 included
    acc[1, :257, 3], acc[1, :257, :3] = n, (255 * n.astype(np.int64))[:, None]   # sum = 255 n
    acc[2, :257, 3], acc[2, :257, :3] = n, (n // 2)[:, None]          # the first sum that rounds up
    acc[3, :257, 3], acc[3, :257, :3] = n, np.maximum(n // 2, 1)[:, None] - 1    # the last that does not
    acc[4, :3] = [(0, 0, 0, 0), (255, 0, 1, 1), (65280, 32640, 128, 256)]
    assert set(np.unique(acc[:, :, 3])) == set(range(257))
    want = rc.accum_resolve(acc)
    assert want[4, :3].tolist() == [[0, 0, 0], [255, 0, 1], [255, 128, 1]]
    d_acc = torch.from_numpy(acc.view(np.int16)).cuda()
    d_out = torch.full((side, side, 3), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.accum_resolve_device(d_acc.data_ptr(), side, side, d_out.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), want)
    # an odd size on a torch stream: the last block is partly outside
    stream = torch.cuda.Stream()
    small = np.ascontiguousarray(acc[:13, :37])
    with torch.cuda.stream(stream):
        d_acc = torch.from_numpy(small.view(np.int16)).pin_memory().cuda(non_blocking=True)
        d_out = torch.zeros((13, 37, 3), dtype=torch.uint8, device="cuda")
        rc.accum_resolve_device(d_acc.data_ptr(), 37, 13, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), rc.accum_resolve(small))


def test_saturation(scenes, torch):
    """n in {250, 251, 255, 256}: passes of 1, 2 and 6 samples change exactly the pixels with
    n + count <= 256 and count the others, over every pixel and over the edge list."""
    rng = np.random.default_rng(9)
    w, h = 33, 17
    g, pts = rc.SAMPLE_SEQS["hier8"]
    big = big_image(scenes, "quadric", g, w, h, 6, "fast")
    n = rng.choice(np.array([250, 251, 255, 256]), size=(h, w))
    acc_in = np.zeros((h, w, 4), np.uint16)
    acc_in[:, :, :3] = rng.integers(0, 256, size=(h, w, 3)) * n[:, :, None]
    acc_in[:, :, 3] = n
    out_in = half_flat_image(rng, h, w)
    mask = rc.edge_mask(out_in, T)
    for count, free in ((1, (250, 251, 255)), (2, (250, 251)), (6, (250,))):
        for t in (0, T):
            acc, out, active, sat = rc.accum_step(acc_in, out_in, big, g, pts[3:3 + count], t)
            m = mask if t else np.ones((h, w), bool)
            assert active == m.sum() and sat == (m & ~np.isin(n, free)).sum() and 0 < sat < active
            changed = (acc != acc_in).any(axis=2)
            np.testing.assert_array_equal(changed, m & np.isin(n, free))
            st = State(torch, w, h, acc_in, out_in)
            st.run(scenes["quadric"], "hier8", 3, count, t=t)
            check_state(st, acc, out, f"count {count} t {t}")
            assert rc.accum_stats() == {"passes": 1, "active_pixels": active, "saturated": sat,
                                        "rays": (active - sat) * count}


@pytest.mark.parametrize("dense,t", [(1, 0), (4, 0), (1, 16), (2, 16)])
def test_host_entry_vs_oracle(dense, t, scenes):
    for name in SCENES:
        for seqname, (w, h), mode, depth in (("queens8", (64, 48), "fast", 6),
                                             ("rgss4", (33, 17), "fast", 6),
                                             ("queens8", (7, 3), "cuda", 50)):
            g, pts = rc.SAMPLE_SEQS[seqname]
            big = big_image(scenes, name, g, w, h, depth, mode)
            want = rc.accum_run(big, g, pts, dense, t)
            tim = {}
            got = rc.render_accum(scenes[name], w, h, seqname, dense, t, depth=depth, mode=mode,
                                  timing=tim)
            tag = f"{name} {seqname} {w}x{h} {mode} dense {dense} t {t}"
            np.testing.assert_array_equal(got, want, err_msg=tag)
            st = rc.accum_stats()
            assert st["passes"] == 1 + len(pts) - dense and st["saturated"] == 0, tag
            # the rays of the whole call, from the contract's passes
            acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
            acc, out, active, _ = rc.accum_step(acc, out, big, g, pts[:dense], 0, reset=True)
            rays = active * dense
            for k in range(dense, len(pts)):
                acc, out, active, _ = rc.accum_step(acc, out, big, g, pts[k:k + 1], t)
                rays += active
            assert st["rays"] == rays == int(acc[:, :, 3].sum()), tag
            assert st["active_pixels"] == active, tag
            assert tim["kernel_ms"] > 0.0 and tim["zero_normalize"] >= 0, tag


def test_host_entry_chunks(scenes):
    """More than 16 dense samples go in chunks: all 64 of hier8 are the ssaa = 8 image."""
    sc = scenes["quadric"]
    want = rc.render(sc, 7, 3, depth=6, mode="fast", ssaa=8)
    np.testing.assert_array_equal(rc.render_accum(sc, 7, 3, "hier8", depth=6, mode="fast"), want)
    assert rc.accum_stats() == {"passes": 4, "active_pixels": 21, "saturated": 0, "rays": 64 * 21}
    np.testing.assert_array_equal(rc.render_accum(sc, 7, 3, "hier8", 40, depth=6, mode="fast"),
                                  want)
    assert rc.accum_stats()["passes"] == 3 + 24


# ---- the per-device state the sampling features share
W, H, DEPTH = 64, 48, 3


def raises(*getters):
    for g in getters:
        with pytest.raises(RuntimeError):
            g()


@pytest.fixture()
def bufs(torch):
    rates = np.array(rc.RATE_VALUES, dtype=np.uint8)[np.arange(W * H) % len(rc.RATE_VALUES)]
    d_rates = torch.from_numpy(rates.reshape(H, W)).cuda()
    d_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_rates, d_out


def test_one_event_set_one_owner(scenes, torch, bufs):
    """Outside a profiling window every frame records event set 0: an accumulation pass takes the
    spans from the pattern frame before it and gives them up to the rate-map frame after it; the
    families' counts are untouched by any of it."""
    sc = scenes["simple"]
    d_rates, d_out = bufs
    rc.render_pattern_device(sc, W, H, "rgss4", d_out.data_ptr(), threshold=0, depth=DEPTH,
                             mode="fast")
    rc.pattern_phase_ms()
    pattern = rc.pattern_stats()
    st = State(torch, W, H)
    st.run(sc, "hier4", 0, 3, reset=True, depth=DEPTH)
    st.run(sc, "hier4", 3, 2, t=T, depth=DEPTH)
    ms = rc.accum_phase_ms()
    assert ms["mark"] > 0.0 and ms["shoot"] > 0.0
    raises(rc.pattern_phase_ms)
    accum = rc.accum_stats()
    assert accum["passes"] == 1 and 0 < accum["active_pixels"] < W * H
    assert accum["rays"] == 2 * accum["active_pixels"]
    rc.render_rates_device(sc, W, H, d_rates.data_ptr(), d_out.data_ptr(), depth=DEPTH,
                           mode="fast")
    rc.rate_phase_ms()
    raises(rc.accum_phase_ms)
    rate = rc.rate_stats()
    # an adaptive and a pattern frame with a threshold: both use the edge list's buffer
    rc.render_device(sc, W, H, d_out.data_ptr(), depth=DEPTH, mode="fast", ssaa=2, adaptive=16,
                     timing={})
    adaptive = rc.adaptive_stats()
    rc.render_pattern_device(sc, W, H, "rgss4", d_out.data_ptr(), threshold=32, depth=DEPTH,
                             mode="fast")
    listed = rc.pattern_stats()
    assert rc.accum_stats() == accum
    # and theirs survive an accumulation pass
    st.run(sc, "hier4", 5, 1, t=T, depth=DEPTH)
    raises(rc.pattern_phase_ms, rc.adaptive_phase_ms, rc.rate_phase_ms)
    assert rc.accum_stats()["passes"] == 1
    assert rc.adaptive_stats() == adaptive and rc.rate_stats() == rate
    assert rc.pattern_stats() == listed and listed != pattern
    torch.cuda.synchronize()


def test_profiling_window_keeps_two_owners(scenes, torch):
    """Inside a profiling window consecutive frames record different event sets, so the pattern
    frame's spans stay readable, unchanged, after an accumulation pass."""
    sc = scenes["simple"]
    st = State(torch, W, H)
    rc.profile_begin()
    try:
        rc.render_pattern_device(sc, W, H, "rgss4", st.d_out.data_ptr(), threshold=0, depth=DEPTH,
                                 mode="fast")
        before = rc.pattern_phase_ms()
        st.run(sc, "hier4", 0, 1, reset=True, depth=DEPTH)
        ms = rc.accum_phase_ms()
        assert ms["mark"] == 0.0 and ms["shoot"] > 0.0
        assert rc.pattern_phase_ms() == before
    finally:
        stats = rc.profile_end()
    torch.cuda.synchronize()
    assert stats["calls"] == 2 and stats["parity"] == 0
