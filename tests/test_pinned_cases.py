"""The cases of tests/test_gpu_pinned.py are what they claim to be (no GPU): the chosen images
hold both kinds of phase C wave — one carry-in in every lane (the table's path) and mixed (the
per-lane path) — and the constructed scenes have the properties the table's host switch reads."""
import ctypes

import numpy as np
import pytest

import pinned_cases as pn
from helpers import oracle_render, rc, scene_path


@pytest.mark.parametrize("name,size,want", [("quadric", 256, (53, 113)), ("quadric2", 256, (7, 732))])
def test_images_hold_both_kinds_of_wave(name, size, want):
    """k_dep_chunks' waves at 256^2, depth 6, in list order: (uniform, all)."""
    s = rc.Scene.from_file(scene_path(name))
    uniform, mixed = pn.wave_census(s, size, size)
    print(f"[pinned_cases] {name} {size}^2: {uniform} uniform waves of {uniform + mixed}")
    assert (uniform, uniform + mixed) == want
    assert uniform > 0 and mixed > 0


def test_small_images_reach_phase_c():
    """The small and odd-shaped images have DEP entries that hit at their carry-in (their waves
    are partial ones)."""
    s = rc.Scene.from_file(scene_path("quadric"))
    for w, h in ((64, 64), (7, 3), (1, 4096), (333, 517)):
        uniform, mixed = pn.wave_census(s, w, h)
        print(f"[pinned_cases] quadric {w}x{h}: {uniform} uniform waves of {uniform + mixed}")
        assert uniform + mixed > 0, (w, h)


def test_image_scenes_take_the_table():
    """All dep_fast; the reflection example's 15 shapes are more than the table's rows, so that
    image is the whole-frame case of a scene that keeps the per-lane code."""
    for name in sorted({n for n, _, _ in pn.IMAGES}):
        n, m, dep_fast, fits = pn.scene_facts(rc.Scene.from_file(scene_path(name)))
        assert dep_fast and fits == (name != "reflection"), (name, n, m, dep_fast, fits)


def test_constructed_scenes():
    q = rc.Scene.from_file(scene_path("quadric"))
    a, b = np.array((1.0, 2.0, -3.0), np.float32), np.array((0.1, -0.7, -6.5), np.float32)
    s = pn.text_scene("facts_light", pn.LIGHT_ROWS(a, b))
    assert pn.scene_facts(s) == (5, 4, True, True)
    assert oracle_render(s, 8, 8, 6, "parity")[1]["parity_defined"]
    # the lights sit exactly where they were put
    lights, p = [], ctypes.cast(s.js.lights_list, ctypes.c_void_p).value
    while p:
        rec = rc.LightT.from_address(p)
        lights.append(tuple(np.float32(rec.position[j]) for j in range(3)))
        p = rec.next
    assert tuple(a) in lights and tuple(b) in lights, lights
    assert pn.scene_facts(pn.text_scene("facts_shape", pn.SHAPE_ROWS)) == (3, 2, True, True)
    assert pn.scene_facts(pn.big_scene("pairs", 8, 9)) == (8, 9, True, False)
    assert pn.scene_facts(pn.big_scene("shapes", 9, 2)) == (9, 2, True, False)
    n, m, dep_fast, fits = pn.scene_facts(pn.lit_phantom_scene())
    assert fits and not dep_fast
    assert pn.scene_facts(q)[2:] == (True, True)
