"""The infrastructure of tests/svgf_schedule.py, held to account on the CPU: the premise of its interpreter (on the exact inputs the
a-trous filter is the identity), the interpreter against the oracle's own port of the reference's host loop, and the liveness helper
against answers worked out by hand."""
import numpy as np
import pytest

from tests import svgf_schedule as ss
from tests.helpers import simple_pfd
from tests.svgf_schedule import A, B, T

SIZES = [(72, 40), (133, 19), (134, 19)]


@pytest.mark.parametrize("W,H", SIZES)
def test_atrous_is_the_identity_on_the_exact_inputs(oracle, W, H):
    """Ids (x mod 9) + 9 (y mod 9), equal normals: a tap k * step away (k = 1, 2) on either axis has another id unless 9 divides the step,
    so oracle.svgf_atrous returns its input bit for bit, variance channels included -- for every step the bodies use, with the display
    size of the image and with the smaller one of H8."""
    normals, _, _ = ss.exact_inputs(W, H)
    image = ss.random_pool(W, H, seed=3)["a"]
    assert len(np.unique(image)) > 500
    for display in (None, (W - 5, H - 3)):
        pfd = simple_pfd(W, H)
        if display:
            pfd["display_size"] = list(display)
        for step in ss.STEPS:
            assert step % 9 != 0
            assert np.array_equal(oracle.svgf_atrous(pfd, normals, image, step), image), f"step {step}, display size {display}"


@pytest.mark.parametrize("W,H", SIZES)
def test_a_pool_image_blitted_into_the_normals_keeps_the_filter_the_identity(oracle, W, H):
    """A body may blit a storage image into Normals.  The exact pool's four-channel images carry ids of their own in the fourth channel
    (random_pool(ids=True)), so the filter stays the identity with any of them as the normals image -- also with one a partial dispatch
    has put together from two of them -- and `every_tap_is_rejected`, which the interpreter asks at every dispatch, says so; of an
    image without ids it says no."""
    pool = ss.random_pool(W, H, seed=1, ids=True)
    mixed = pool["c"].copy()
    mixed[:H // 2, :W // 3] = pool["history"][:H // 2, :W // 3]
    image = pool["a"]
    for normals in [pool[name] for name in ss.STORAGE_RGBA] + [mixed]:
        for step in ss.STEPS:
            assert ss.every_tap_is_rejected(normals, step)
            assert np.array_equal(oracle.svgf_atrous(simple_pfd(W, H), normals, image, step), image)
    assert not ss.every_tap_is_rejected(ss.random_pool(W, H, seed=1)["a"], 1)
    assert not ss.every_tap_is_rejected(ss.live_inputs(W, H)[0], 2)


@pytest.mark.parametrize("W,H", SIZES)
def test_atrous_filters_on_the_live_inputs(oracle, W, H):
    """The other comparison's premise: on `live_inputs` the filter changes most pixels of a pool image at every step the bodies use, so a
    dispatch that is skipped, repeated or fed another image shows there.  (svgf_cases.live_taps keeps >= 90 % of the pixels changing at
    the step it is drawn for, 2; at the other steps a tap 2 * step away still shares its centre's 24-pixel block for part of the image.)"""
    normals, _, _ = ss.live_inputs(W, H)
    image = ss.random_pool(W, H, seed=2)["a"]
    for step in ss.STEPS:
        out = oracle.svgf_atrous(simple_pfd(W, H), normals, image, step)
        changed = float((out != image).any(-1).mean())
        print(f"{W}x{H} step {step}: {changed:.3f} of the pixels change")
        assert changed >= (0.9 if step <= 2 else 0.25), (step, changed)


@pytest.mark.parametrize("W,H", SIZES)
def test_interpreter_equals_the_oracles_host_loop_on_the_reference_body(oracle, W, H):
    """The reference's body through `interpret` (identity for the filter, array copies for the blits) against oracle.SVGF, which runs
    orc_svgf_atrous and memcpy in the order of hybrid_render_path.cpp:291-328: four frames from zeroed images, all five persistent images
    and Denoised bit for bit after every frame."""
    inputs = ss.exact_inputs(W, H)
    zero = {name: np.zeros((H, W, ss.CHANNELS[name]), np.uint16) for name in ss.POOL}
    frames = ss.interpret((W, H), [ss.reference_body()] * 4, inputs, zero, oracle, every_frame=True)
    svgf = oracle.SVGF(W, H)
    for f, got in enumerate(frames):
        denoised = svgf.frame(simple_pfd(W, H), *inputs)
        want = dict(Denoised=denoised, a=svgf.image(0), b=svgf.image(1), prev_normals=svgf.image(2), history=svgf.image(3), moments=svgf.image(4))
        for name, ref in want.items():
            assert np.array_equal(got[name], ref), f"frame {f}: {name}"
    assert got["history"].any() and got["moments"].any() and np.array_equal(got["prev_normals"], inputs[0])


def test_unread_dispatches_by_hand():
    # the reference's body: only the fifth iteration (index 6: T, A, B, A, A, A, [A], B, B) writes an image nothing reads afterwards
    assert ss.unread_dispatches(ss.reference_body()) == [6]
    # b is read by the blit although a dispatch rewrites it in between: "no later command reads" asks no more; c and the last b are unread
    body = [A("a", "b", 1), A("c", "b", 2), B("b", "s"), A("s", "c", 1), A("a", "b", 4)]
    assert ss.unread_dispatches(body) == [3, 4]
    # svgf.comp reads the history and the previous normals; a blit onto itself reads nothing; a dispatch's own source is no later read
    body = [A("a", "history", 1), A("a", "prev_normals", 2), A("b", "s", 1), B("s", "s"), T(), A("s", "c", 2), A("c", "a", 1)]
    assert ss.unread_dispatches(body) == [6]
    assert ss.unread_dispatches(body[:4]) == [0, 1, 2]


def test_exemptions_and_structure_by_hand():
    # within one body: what an unread dispatch wrote last; a later whole write from clean images ends the exemption
    assert ss.exempt_images([[A("a", "b", 1), A("b", "c", 2), A("s", "b", 4)]]) == {"b", "c"}
    assert ss.exempt_images([[A("a", "c", 1), B("a", "c")]]) == set()
    assert ss.exempt_images([[A("a", "c", 1), A("a", "c", 1, 2, 2), B("c", "s")]]) == set()
    # across frames the exemption travels with the data
    assert ss.exempt_images([[A("a", "b", 1), A("b", "c", 2)], [B("c", "s")]]) == {"c", "s"}
    assert ss.exempt_images([[A("a", "b", 1), A("b", "c", 2)], [A("a", "c", 1), B("c", "s")]]) == set()
    assert ss.fuses_by_structure([A("a", "b", 1), B("b", "s")])
    assert not ss.fuses_by_structure([A("a", "b", 1), B("b", "s"), A("s", "c", 1)])
    assert not ss.fuses_by_structure([A("a", "b", 1, 3, 3), B("b", "s")])
    assert not ss.fuses_by_structure([A("a", "b", 1), T(), B("b", "history")])
    # (the reference's body: svgf.comp reads the history, and the blit into Denoised does not directly follow its dispatch)
    assert not ss.fuses_by_structure(ss.reference_body())


def test_random_bodies_are_what_they_are_meant_to_be():
    bodies = ss.random_bodies()
    assert bodies == ss.random_bodies() and len(bodies) == 40
    assert all(4 <= len(b) <= 9 for b in bodies)
    last_dispatch = [max((i for i, c in enumerate(b) if isinstance(c, A)), default=-1) for b in bodies]
    ends_unread = [i >= len(b) - 2 and i in ss.unread_dispatches(b) for b, i in zip(bodies, last_dispatch)]
    assert sum(ends_unread) >= 20
    assert all(ss.keeps_ids([b, b]) for b in bodies)
    assert sum(any(isinstance(c, B) and c.dst == "Normals" for c in b) for b in bodies) >= 5
    assert sum(ss.fuses_by_structure(b) for b in bodies) >= 5
    assert sum(any(isinstance(c, T) for c in b) for b in bodies) >= 5
    assert sum(any(isinstance(c, B) and c.src == "Normals" for c in b) and e for b, e in zip(bodies, ends_unread)) >= 20
