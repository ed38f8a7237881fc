"""The per-device state the sampling features share (adaptive supersampling, rate maps, sparse
patterns, filtered two-pass frames): which family's phase spans a getter may still read after
another family's frame has taken the event set, and that each family's counts outlive the
others' frames.  No image is compared here (the families' own tests do that), so no oracle is
needed."""
import math

import numpy as np
import pytest

from helpers import rc, scene_path

pytestmark = pytest.mark.gpu

W, H, DEPTH = 64, 48, 3
PHASE_GETTERS = (rc.adaptive_phase_ms, rc.rate_phase_ms, rc.filter_phase_ms, rc.pattern_phase_ms)


@pytest.fixture(scope="module")
def scene():
    return rc.Scene.from_file(scene_path("simple"))


@pytest.fixture()
def bufs():
    torch = pytest.importorskip("torch")
    rates = np.array(rc.RATE_VALUES, dtype=np.uint8)[np.arange(W * H) % len(rc.RATE_VALUES)]
    assert sorted(set(rates.tolist())) == sorted(rc.RATE_VALUES)   # the map holds every rate
    d_rates = torch.from_numpy(rates.reshape(H, W)).cuda()
    d_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_rates, d_out


def spans(getter, keys):
    """The getter's spans: exactly `keys`, each finite and not negative."""
    ms = getter()
    assert sorted(ms) == sorted(keys), ms
    assert all(math.isfinite(v) and v >= 0.0 for v in ms.values()), ms
    return ms


def raises(*getters):
    for g in getters:
        with pytest.raises(RuntimeError):
            g()


def test_one_event_set_one_owner(scene, bufs):
    """Outside a profiling window every frame records event set 0, so each family's frame takes
    the spans from the family before it, and a timed plain frame takes them from all four; the
    families' counts are untouched by any of it."""
    d_rates, d_out = bufs
    # 1. a timed adaptive frame
    rc.render_device(scene, W, H, d_out.data_ptr(), depth=DEPTH, mode="fast", ssaa=2, adaptive=16,
                     timing={})
    spans(rc.adaptive_phase_ms, ("render", "mark", "refine"))
    adaptive = rc.adaptive_stats()
    assert 0 < adaptive["refined_pixels"] < W * H
    # 2. a rate-map frame
    rc.render_rates_device(scene, W, H, d_rates.data_ptr(), d_out.data_ptr(), depth=DEPTH,
                           mode="fast")
    spans(rc.rate_phase_ms, ("render", "refine"))
    raises(rc.adaptive_phase_ms)
    rate = rc.rate_stats()
    assert all(n > 0 for n in rate["pixels"].values()) and rate["invalid"] == 0
    # 3. a dense pattern frame
    rc.render_pattern_device(scene, W, H, "rgss4", d_out.data_ptr(), threshold=0, depth=DEPTH,
                             mode="fast")
    ms = spans(rc.pattern_phase_ms, ("render", "mark", "refine"))
    assert ms["mark"] == 0.0 and ms["refine"] == 0.0
    raises(rc.rate_phase_ms)
    pattern = rc.pattern_stats()
    assert pattern == {"refined_pixels": W * H, "rays": 4 * W * H}
    # 4. a timed filtered frame
    rc.render_filtered_device(scene, W, H, rc.filter_tent(2), 2, d_out.data_ptr(), depth=DEPTH,
                              mode="fast", timing={})
    spans(rc.filter_phase_ms, ("render", "filter"))
    raises(rc.pattern_phase_ms)
    # 5. a timed plain frame
    rc.render_device(scene, W, H, d_out.data_ptr(), depth=DEPTH, mode="fast", timing={})
    raises(*PHASE_GETTERS)
    # 6. each family's counts survive the others' frames
    assert rc.adaptive_stats() == adaptive
    assert rc.rate_stats() == rate
    assert rc.pattern_stats() == pattern


def test_profiling_window_keeps_two_owners(scene, bufs):
    """Prediction from DevCtx: rc_profile_begin zeroes prof_calls, and inside the window call k
    records set k % kEvSets (64 sets).  The adaptive frame is call 0 (set 0), the rate-map frame
    call 1 (set 1); a frame only takes the spans of an owner that points at the set it records,
    so both getters work after both frames, and the adaptive spans, read from events that were
    not recorded anew, are the very same numbers before and after the rate-map frame."""
    d_rates, d_out = bufs
    rc.profile_begin()
    try:
        rc.render_device(scene, W, H, d_out.data_ptr(), depth=DEPTH, mode="fast", ssaa=2,
                         adaptive=16, timing={})
        before = spans(rc.adaptive_phase_ms, ("render", "mark", "refine"))
        rc.render_rates_device(scene, W, H, d_rates.data_ptr(), d_out.data_ptr(), depth=DEPTH,
                               mode="fast")
        spans(rc.rate_phase_ms, ("render", "refine"))
        assert spans(rc.adaptive_phase_ms, ("render", "mark", "refine")) == before
    finally:
        stats = rc.profile_end()
    assert stats["calls"] == 2 and stats["parity"] == 0
