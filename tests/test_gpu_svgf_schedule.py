"""Whatever a compute pass's body is, the library gives what the body's commands give one after the other.

The SVGF pass records its commands and rewrites the list (csrc/kernels_svgf.hip, copy_image_rows and flush_recorded): a blit becomes a
second store of the a-trous launch that produced its source, the normals blit a store of a launch that reads the normals, a dispatch
nothing reads is elided ("svgf_elide_unread") or issued last on the side stream with its inputs swapped for copies
("svgf_async_unread").  Every rewrite is guarded by a read / write analysis over image pointers.  Here that analysis meets bodies built
to trip it (R, H1 ... H20) and 40 seeded random ones, at three sizes, under six option sets and both a-trous kernel forms:

  * on `exact_inputs` every option set, the in-order one included, equals svgf_schedule.interpret on every pool image and Denoised,
    bit for bit, after the last frame;
  * on `live_inputs` (real filtering, real texels in the fused stores) every optimised set equals the in-order device run bit for bit.

Under "svgf_elide_unread" the images svgf_schedule.exempt_images names are not compared -- nothing else is left out.  The launch counts
in the docstrings are derived by hand from the rules in kernels_svgf.hip and asserted; with VHR_SVGF_SCHEDULE_COUNTS=<file> in the
environment the measured counts of every run are written there (profiles/svgf_schedule.txt is such a file).

Sizes: 72 x 40 has two tile columns, the second partial; 133 x 19 has three and fewer rows than one 8-row tile group at step 4 -- and
its images are no whole number of 16-byte units, so a blit that stays a copy goes through hipMemcpyAsync instead of the copy kernel:
the other copy path, and a `blit` kernel count of 0 whatever the body.  134 x 19 is that shape with whole 16-byte units in its four-
channel images: there and at 72 x 40 the blit counts of the docstrings are asserted and tell a fused blit from a copy."""
import os

import numpy as np
import pytest

from tests import svgf_schedule as ss
from tests.svgf_schedule import A, B, T

pytestmark = pytest.mark.gpu

SIZES = [(72, 40), (133, 19), (134, 19)]
# (a name left out keeps the library's default: "svgf_elide_unread" 0, "svgf_async_unread" 1, "frames_in_flight" 1)
OPTION_SETS = {
    "in_order": dict(fuse_blits=0, svgf_elide_unread=0, svgf_async_unread=0),
    "fused": dict(fuse_blits=1, svgf_async_unread=0),
    "fused_async": dict(fuse_blits=1, svgf_async_unread=2),
    "async": dict(fuse_blits=0, svgf_async_unread=2),
    "fused_elide": dict(fuse_blits=1, svgf_elide_unread=1),
    "fused_async_2_in_flight": dict(fuse_blits=1, svgf_async_unread=2, frames_in_flight=2),          # the deferral switches itself off
}
N = B("Normals", "prev_normals")          # the pass's copy of the normals: without one in the body nothing goes to the side stream


class _Runners:
    def __init__(self):
        self.cache, self.counts = {}, []

    def get(self, size, set_name, variant, display=None):
        key = (size, set_name, variant, display)
        if key not in self.cache:
            self.cache[key] = ss.DeviceRunner(size, dict(OPTION_SETS[set_name], atrous_variant=variant), display)
        return self.cache[key]

    def close(self, display="all"):
        for key in [k for k in self.cache if display == "all" or k[3] == display]:
            self.cache.pop(key).close()


@pytest.fixture(scope="module")
def runners():
    """One context per (size, option set, kernel form, display size), reused for body after body."""
    r = _Runners()
    yield r
    r.close()
    path = os.environ.get("VHR_SVGF_SCHEDULE_COUNTS")
    if path:
        with open(path, "w") as f:
            f.write("# launches per run (all frames): body, size, a-trous kernel form, option set -> blit svgf_atrous svgf_atrous_async svgf_temporal\n")
            f.writelines(line + "\n" for line in r.counts)


def _differences(got, want, skip, what):
    return [f"{what}: {name} differs in {int((got[name] != want[name]).any(-1).sum())} pixels" for name in ss.POOL
            if name not in skip and not np.array_equal(got[name], want[name])]


def _judge(runners, oracle, name, frames, size, expect=None, display=None):
    """Both comparisons and the launch counts of one run (a list of bodies, no synchronisation between frames) under every option set and
    kernel form.  expect: hand-derived launches over all frames, dict(blit=..., async_fused=..., async_unfused=...) -- `blit` with
    "fuse_blits" 1 (without, every blit of the bodies is a kernel), `svgf_atrous_async` under the sets "fused_async" and "async"."""
    W, H = size
    exact, live = ss.exact_inputs(W, H), ss.live_inputs(W, H)
    pool_exact, pool_live = ss.random_pool(W, H, seed=1, ids=True), ss.random_pool(W, H, seed=2, prev_normals=live[0])
    truth = ss.interpret(size, frames, exact, pool_exact, oracle, display)
    exempt = ss.exempt_images(frames)
    commands = [c for body in frames for c in body]
    # issue_copy launches its copy kernel for images of whole 16-byte units and hands every other one to hipMemcpyAsync, which no kernel
    # count sees: 133 x 19 texels of 8 or 4 bytes are such images, so there every blit that is not fused counts 0
    copy_kernel = lambda name: (W * H * 2 * ss.CHANNELS[name]) % 16 == 0          # noqa: E731
    n_blits = sum(isinstance(c, B) and c.src != c.dst and copy_kernel(c.src) for c in commands)
    if expect is not None:          # (a two-channel blit is never fused: where its image takes the hipMemcpyAsync path it counts 0 in every set)
        rg_memcpy = sum(isinstance(c, B) and c.src != c.dst and ss.CHANNELS[c.src] == 2 and not copy_kernel(c.src) for c in commands)
        expect = dict(expect, blit=expect["blit"] - rg_memcpy if copy_kernel("a") else 0)
    n_atrous, n_temporal = sum(isinstance(c, A) for c in commands), sum(isinstance(c, T) for c in commands)
    failures = []
    for variant in (0, 1):
        base, blits = None, {}
        for set_name, opts in OPTION_SETS.items():
            what = f"{name} {W}x{H} kernel form {variant} {set_name}"
            r = runners.get(size, set_name, variant, display)
            skip = exempt if opts.get("svgf_elide_unread") else ()
            got, _, counts = r.run(frames, exact, pool_exact)
            failures += _differences(got, truth, skip, what + ", exact inputs against the interpreter")
            got_live, _, counts_live = r.run(frames, live, pool_live)
            if set_name == "in_order":
                base = got_live
            else:
                failures += _differences(got_live, base, skip, what + ", live inputs against the in-order run")
            runners.counts.append(f"{name} {W}x{H} {variant} {set_name} -> " + " ".join(str(counts[k]) for k in ss.KERNEL_KINDS) +
                                  f"  (images compared: {len(ss.POOL) - len(set(skip))} of {len(ss.POOL)})")
            blits[set_name] = counts["blit"]
            # ---- launch counts ----
            if counts_live != counts:
                failures.append(f"{what}: the schedule depends on the images' contents: {counts} / {counts_live}")
            if counts["svgf_temporal"] != n_temporal:
                failures.append(f"{what}: {counts['svgf_temporal']} svgf.comp launches for {n_temporal} dispatches")
            ran = counts["svgf_atrous"] + counts["svgf_atrous_async"]
            if ran > n_atrous or (ran < n_atrous and not opts.get("svgf_elide_unread")):
                failures.append(f"{what}: {ran} a-trous launches for {n_atrous} dispatches")
            defers = opts.get("svgf_async_unread") == 2 and "frames_in_flight" not in opts
            want_async = 0 if not defers else None if expect is None else expect["async_fused" if opts["fuse_blits"] else "async_unfused"]
            if want_async is not None and counts["svgf_atrous_async"] != want_async:
                failures.append(f"{what}: {counts['svgf_atrous_async']} launches on the side stream, {want_async} expected")
            want_blit = n_blits if not opts["fuse_blits"] else None if expect is None else expect["blit"]
            if want_blit is not None and counts["blit"] != want_blit:
                failures.append(f"{what}: {counts['blit']} blit kernels, {want_blit} expected")
        # non-vacuity from the body's structure alone: such a blit is fused, whatever else the body holds
        if copy_kernel("a") and any(ss.fuses_by_structure(body) for body in frames):
            for set_name, opts in OPTION_SETS.items():
                if opts["fuse_blits"] and not blits[set_name] < blits["in_order"]:
                    failures.append(f"{name} {W}x{H} kernel form {variant} {set_name}: no blit was fused ({blits[set_name]} kernels, in order {blits['in_order']})")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40]) + "\nbodies: " + " | ".join(ss.show(b) for b in frames)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_r_the_reference_schedule(runners, oracle, size):
    """R, what HybridRenderPath records, two frames.  No hazard: the three blits are fused (b -> history into iteration 0, Normals ->
    prev_normals into iteration 0 too -- the earliest dispatch behind svgf.comp, which reads prev_normals --, a -> Denoised into iteration
    3): 0 blit kernels, 3 per frame without fusion.  Iteration 4 is unread and has copies of both inputs: one side-stream launch per
    frame, with and without fusion (the unfused normals blit comes after it).  Then once more with a host synchronisation after every
    frame, every frame against the interpreter."""
    frames = [ss.reference_body()] * 2
    _judge(runners, oracle, "R", frames, size, dict(blit=0, async_fused=2, async_unfused=2))
    W, H = size
    exact, pool = ss.exact_inputs(W, H), ss.random_pool(W, H, seed=1, ids=True)
    truth = ss.interpret(size, frames, exact, pool, oracle, every_frame=True)
    for set_name in ("fused_async", "fused_elide"):
        _, per_frame, _ = runners.get(size, set_name, 1).run(frames, exact, pool, sync_between_frames=True)
        for f, (got, want) in enumerate(zip(per_frame, truth)):
            skip = ss.exempt_images(frames[:f + 1]) if set_name == "fused_elide" else ()
            assert not _differences(got, want, skip, f"R {set_name} frame {f}")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h1_read_before_overwrite_on_the_blit_destination(runners, oracle, size):
    """H1: A a->b; A s->c; B b->s.  Fused into the first dispatch, the blit would let the second one read the new s: it must stay a
    copy.  1 blit kernel; nothing on the side stream (the body copies no normals)."""
    _judge(runners, oracle, "H1", [[A("a", "b", 1), A("s", "c", 2), B("b", "s")]], size, dict(blit=1, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h2_two_writes_to_the_destination(runners, oracle, size):
    """H2: A a->b; B c->s; B b->s.  s ends as b: the second blit may not move in front of the first, which no dispatch can take (c has
    no producer in the body).  2 blit kernels."""
    _judge(runners, oracle, "H2", [[A("a", "b", 1), B("c", "s"), B("b", "s")]], size, dict(blit=2, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h3_source_rewritten(runners, oracle, size):
    """H3: A a->b step 1; A c->b step 2; B b->s.  s is the SECOND dispatch's output; the blit is its second store: 0 blit kernels."""
    _judge(runners, oracle, "H3", [[A("a", "b", 1), A("c", "b", 2), B("b", "s")]], size, dict(blit=0, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h4_two_blits_of_one_source(runners, oracle, size):
    """H4: A a->b; B b->s; B b->Denoised.  A launch has one second store: the first blit is fused, the other one a copy.  1 blit kernel."""
    _judge(runners, oracle, "H4", [[A("a", "b", 1), B("b", "s"), B("b", "Denoised")]], size, dict(blit=1, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h5_source_written_by_svgf_comp(runners, oracle, size):
    """H5: T; B a->s; B moments->m2.  svgf.comp has no second store and a two-channel image is never fused: 2 blit kernels.  The second
    copies the NEW moments: the image's twin buffers are flipped when svgf.comp is recorded."""
    _judge(runners, oracle, "H5", [[T(), B("a", "s"), B("moments", "m2")]], size, dict(blit=2, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h6_the_normals_blit_may_not_pass_a_reader_of_its_destination(runners, oracle, size):
    """H6: A a->b; T; B Normals->prev_normals -- svgf.comp reads the old prev_normals behind the only dispatch that could take the store:
    1 blit kernel.  And T; A a->b; B Normals->prev_normals; T -- the dispatch behind the first svgf.comp takes it (0 blit kernels) and the
    second svgf.comp reads the new normals.  Nothing goes to the side stream: svgf.comp rewrites the unread dispatch's input `a`."""
    _judge(runners, oracle, "H6a", [[A("a", "b", 1), T(), N]], size, dict(blit=1, async_fused=0, async_unfused=0))
    _judge(runners, oracle, "H6b", [[T(), A("a", "b", 1), N, T()]], size, dict(blit=0, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h7_partial_dispatch(runners, oracle, size):
    """H7: A a->b over two x groups and one y group fewer than the image needs; B b->s.  The blit copies texels the dispatch never wrote:
    it cannot be that launch's store.  1 blit kernel."""
    W, H = size
    body = [A("a", "b", 1, ss.groups(W) - 2, ss.groups(H) - 1), B("b", "s")]
    _judge(runners, oracle, "H7", [body], size, dict(blit=1, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h8_display_size_smaller_than_the_image(runners, oracle, size):
    """H8: R and H4 with display_size = (W - 5, H - 3) and whole-image dispatches: the library takes the literal a-trous kernel, which
    carries the fused stores too.  Counts as R and H4."""
    display = (size[0] - 5, size[1] - 3)
    try:
        _judge(runners, oracle, "H8/R", [ss.reference_body()] * 2, size, dict(blit=0, async_fused=2, async_unfused=2), display)
        _judge(runners, oracle, "H8/H4", [[A("a", "b", 1), B("b", "s"), B("b", "Denoised")]], size, dict(blit=1, async_fused=0, async_unfused=0), display)
    finally:
        runners.close(display)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h9_unread_dispatch_whose_input_is_overwritten_later(runners, oracle, size):
    """H9: A a->b; A b->c; A s->b (; B Normals->prev_normals, so that a dispatch may be deferred at all).  A b->c is unread, but issued last
    it would read the third dispatch's b: it stays in place.  The third dispatch is unread too and nothing follows it: that one goes to
    the side stream, 1 launch, with and without fusion.  The normals blit is the first dispatch's store: 0 blit kernels."""
    _judge(runners, oracle, "H9", [[A("a", "b", 1), A("b", "c", 2), A("s", "b", 4), N]], size, dict(blit=0, async_fused=1, async_unfused=1))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h10_a_fused_normals_store_overwrites_the_copy_of_the_input(runners, oracle, size):
    """H10: A a->b step 1; B b->s; A b->a step 2; B Normals->s; A b->c step 1.  The first blit is the first dispatch's second store, so s
    is a copy of b -- until the second blit, a store of the second dispatch, puts the normals there.  The unread A b->c goes to the side
    stream (s is its copy of the normals) and must read b, not s.  0 blit kernels, 1 side-stream launch; without fusion the normals copy
    precedes the dispatch and is not looked for: 0.  (Before this test existed the dispatch filtered the normals image.)"""
    body = [A("a", "b", 1), B("b", "s"), A("b", "a", 2), B("Normals", "s"), A("b", "c", 1)]
    _judge(runners, oracle, "H10", [body], size, dict(blit=0, async_fused=1, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h11_a_fused_copy_of_the_unread_dispatchs_input_is_overwritten_after_it(runners, oracle, size):
    """H11: A a->b; B b->s; A b->c; B a->s (; B Normals->prev_normals).  s is a copy of b when A b->c is recorded and a copy of `a` when
    the pass ends: the deferred dispatch reads b.  B a->s stays a copy (the first dispatch writes s): 1 blit kernel; 1 side-stream launch
    with and without fusion."""
    body = [A("a", "b", 1), B("b", "s"), A("b", "c", 2), B("a", "s"), N]
    _judge(runners, oracle, "H11", [body], size, dict(blit=1, async_fused=1, async_unfused=1))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h12_two_unread_dispatches_in_one_body(runners, oracle, size):
    """H12: A a->b; A b->c; A b->s; B Normals->prev_normals.  Two dispatches nothing reads; the side stream takes one dispatch per pass,
    the first: 1 side-stream launch, the other one in place.  0 blit kernels."""
    _judge(runners, oracle, "H12", [[A("a", "b", 1), A("b", "c", 2), A("b", "s", 2), N]], size, dict(blit=0, async_fused=1, async_unfused=1))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h13_a_side_stream_dispatch_pending_across_frames(runners, oracle, size):
    """H13: frame 0 is A a->b; A b->c; B Normals->prev_normals and leaves A b->c on the side stream; the host does not wait.  Frame 1
    begins with a command that reads what it writes (B c->s; A c->a) or writes it (A a->c): the context's stream has to wait for the side
    stream first.  1 side-stream launch (frame 1's own unread dispatch has no normals copy); blit kernels: the B c->s of frame 1."""
    first = [A("a", "b", 1), A("b", "c", 2), N]
    _judge(runners, oracle, "H13/blit", [first, [B("c", "s")]], size, dict(blit=1, async_fused=1, async_unfused=1))
    _judge(runners, oracle, "H13/read", [first, [A("c", "a", 1)]], size, dict(blit=0, async_fused=1, async_unfused=1))
    _judge(runners, oracle, "H13/write", [first, [A("a", "c", 1)]], size, dict(blit=0, async_fused=1, async_unfused=1))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h14_svgf_comp_twice_in_one_body(runners, oracle, size):
    """H14: T; B a->history; T.  The moments flip twice; the second svgf.comp reads the history the blit wrote and the first one's
    moments.  1 blit kernel (svgf.comp has no second store)."""
    _judge(runners, oracle, "H14", [[T(), B("a", "history"), T()]], size, dict(blit=1, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h15_the_input_is_rewritten_after_its_fused_copy_was_made(runners, oracle, size):
    """H15: A a->b step 1; B b->s; A c->b step 2; B Normals->prev_normals; A b->a.  s is a copy of the FIRST dispatch's b; the unread last
    dispatch reads the second one's.  Both blits are stores of the first dispatch: 0 blit kernels; 1 side-stream launch, and without
    fusion 0 (the normals copy precedes the dispatch).  (Before this test existed the dispatch read s.)"""
    body = [A("a", "b", 1), B("b", "s"), A("c", "b", 2), N, A("b", "a", 1)]
    _judge(runners, oracle, "H15", [body], size, dict(blit=0, async_fused=1, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h16_svgf_comp_overwrites_the_fused_copy_of_the_input(runners, oracle, size):
    """H16: A s->b; B b->a; B Normals->prev_normals; A b->c; T.  `a` is a copy of b until svgf.comp, later in the body, writes its
    integrated image there; the unread A b->c, issued behind it, reads b.  Both blits are stores of the first dispatch: 0 blit kernels; 1
    side-stream launch, without fusion 0.  (Before this test existed the dispatch read svgf.comp's output.)"""
    body = [A("s", "b", 1), B("b", "a"), N, A("b", "c", 2), T()]
    _judge(runners, oracle, "H16", [body], size, dict(blit=0, async_fused=1, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h17_the_unread_dispatch_writes_the_image_that_holds_the_normals_copy(runners, oracle, size):
    """H17: A a->b; B Normals->prev_normals; A b->prev_normals.  The blit is the first dispatch's store, so prev_normals is a copy of the
    normals -- and the unread last dispatch's own output: on the side stream it would read its normals from the image it is writing.  It
    stays in place: 0 side-stream launches, 0 blit kernels.  (Found by a random body; before, the literal kernel's taps read normals
    that other threads had already overwritten: 292 of 2880 pixels differed on the live inputs.)"""
    _judge(runners, oracle, "H17", [[A("a", "b", 1), N, A("b", "prev_normals", 1)]], size, dict(blit=0, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h18_the_unread_dispatch_writes_the_image_that_holds_the_copy_of_its_input(runners, oracle, size):
    """H18: A a->b; B b->c; B Normals->prev_normals; A b->c step 2.  c is a copy of b (the first dispatch's second store) and the unread
    last dispatch's output: reading the copy, it would filter c in place.  It goes to the side stream and reads b: 1 side-stream launch
    (without fusion the normals copy precedes it: 0), 0 blit kernels."""
    body = [A("a", "b", 1), B("b", "c"), N, A("b", "c", 2)]
    _judge(runners, oracle, "H18", [body], size, dict(blit=0, async_fused=1, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h19_the_normals_are_rewritten_after_their_fused_copy_was_made(runners, oracle, size):
    """H19: A a->b; B Normals->prev_normals; B s->Normals; A b->c.  The first blit is the first dispatch's store: prev_normals holds the
    OLD normals.  The second blit puts s into the G-buffer image, and the unread last dispatch filters with those: prev_normals is no
    copy of what it reads, and it stays in place.  0 side-stream launches; B s->Normals stays a copy (the first dispatch reads its
    destination): 1 blit kernel."""
    body = [A("a", "b", 1), N, B("s", "Normals"), A("b", "c", 1)]
    _judge(runners, oracle, "H19", [body], size, dict(blit=1, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_h20_the_normals_are_rewritten_behind_the_unread_dispatch(runners, oracle, size):
    """H20: A a->b; A b->c; B s->Normals; B Normals->prev_normals.  The unread A b->c reads the old normals; the copy the pass makes
    afterwards is one of the NEW ones: the dispatch stays in place, 0 side-stream launches with and without fusion.  Neither blit can
    be a store (no dispatch produced s, and none behind the rewrite reads the normals): 2 blit kernels."""
    body = [A("a", "b", 1), A("b", "c", 2), B("s", "Normals"), N]
    _judge(runners, oracle, "H20", [body], size, dict(blit=2, async_fused=0, async_unfused=0))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("index", range(40))
def test_random_bodies(runners, oracle, size, index):
    """Seeded random bodies (svgf_schedule.random_bodies), the same body for two frames without a host synchronisation between them."""
    body = ss.random_bodies()[index]
    _judge(runners, oracle, f"random{index:02d}", [body, body], size)
