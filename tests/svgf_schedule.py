"""Pass bodies for the SVGF compute pass as data, and three ways to run them (TEST INFRASTRUCTURE, no tests).

A compute pass records its commands and the library rewrites the list before it issues it (csrc/kernels_svgf.hip: blits become stores of
a-trous launches, a dispatch nothing reads is elided or issued last on a side stream).  Whatever it does, a body must give what its
commands give when they run one after the other.  Here a body is a list of three kinds of command over NAMED images:

    T(x_groups, y_groups)               svgf.comp: reads Normals, Motion, Raytraced, prev_normals, history, moments; writes `a` and moments
    A(src, dst, step, x_groups, y_groups)   svgf_atrous_filter.comp: reads Normals and `src`, writes `dst`
    B(src, dst)                         a blit (storage -> storage, storage -> transient or transient -> storage, picked from the names)

(groups None: as many as the image needs.)  A run is a list of bodies, one per frame.

    run_device / DeviceRunner   the library, under a set of options
    interpret                   THE TRUTH: the commands strictly in order on numpy arrays
    unread_dispatches           which dispatches of a body write an image no later command of the body reads

`interpret` needs no a-trous arithmetic: on `exact_inputs` every pixel has the object id (x mod 9) + 9 (y mod 9) and all normals are
equal, so every tap of every step that is no multiple of 9 has another id than its centre and the filter returns its input bit for bit
(tests/test_svgf_schedule.py holds the oracle's filter to that).  svgf.comp is oracle.svgf_temporal, to which the kernel is held bit-exact
(tests/test_gpu_svgf.py)."""
from collections import namedtuple

import numpy as np

from tests import svgf_cases
from tests.helpers import GpuSvgfHarness, simple_pfd, synthetic_svgf_inputs
from vulkanhybridrenderer_amd import abi, lib

T = namedtuple("T", "x_groups y_groups", defaults=(None, None))
A = namedtuple("A", "src dst step x_groups y_groups", defaults=(None, None))
B = namedtuple("B", "src dst")

STORAGE_RGBA = ("a", "b", "c", "s", "prev_normals", "history")
STORAGE_RG = ("moments", "m2")
TRANSIENTS = {"Normals": lib.NORMALS, "Motion": lib.MOTION, "Raytraced": lib.RAYTRACED, "Denoised": lib.DENOISED}
CHANNELS = dict({n: 4 for n in STORAGE_RGBA}, moments=2, m2=2, Normals=4, Motion=4, Raytraced=2, Denoised=4)
POOL = STORAGE_RGBA + STORAGE_RG + ("Denoised",)          # what a run starts from (pool_init) and what it returns
KERNEL_KINDS = ("blit", "svgf_atrous", "svgf_atrous_async", "svgf_temporal")
T_READS = ("Normals", "Motion", "Raytraced", "prev_normals", "history", "moments")
T_WRITES = ("a", "moments")
STEPS = (1, 2, 3, 4, 8, 16)                               # the step sizes the bodies use (3: no tile kernel, the literal one)


def groups(n):
    return (n + 7) // 8


def covered(cmd, W, H):
    """(columns, rows) a dispatch computes."""
    return (W if cmd.x_groups is None else min(W, 8 * cmd.x_groups)), (H if cmd.y_groups is None else min(H, 8 * cmd.y_groups))


def whole(cmd):
    return cmd.x_groups is None and cmd.y_groups is None


def reads(cmd):
    if isinstance(cmd, T):
        return T_READS
    if isinstance(cmd, A):
        return ("Normals", cmd.src)
    return () if cmd.src == cmd.dst else (cmd.src,)


def writes(cmd):
    if isinstance(cmd, T):
        return T_WRITES
    return () if isinstance(cmd, B) and cmd.src == cmd.dst else (cmd.dst,)


def check_body(body):
    for cmd in body:
        if isinstance(cmd, A):
            assert cmd.src in STORAGE_RGBA and cmd.dst in STORAGE_RGBA and cmd.src != cmd.dst and cmd.step in STEPS, cmd
        elif isinstance(cmd, B):
            assert CHANNELS[cmd.src] == CHANNELS[cmd.dst] and not (cmd.src in TRANSIENTS and cmd.dst in TRANSIENTS), cmd
        else:
            assert isinstance(cmd, T), cmd


# ---- liveness: "an a-trous dispatch whose output image no later command of the same pass reads" ----
def unread_dispatches(body):
    """Indices of the dispatches A of `body` whose destination no later command of the body reads."""
    return [i for i, cmd in enumerate(body) if isinstance(cmd, A) and not any(cmd.dst in reads(later) for later in body[i + 1:])]


def exempt_images(frames):
    """The images a run under "svgf_elide_unread" need not agree on.  Within a body: the images written last by an unread dispatch.  The
    option leaves such an image holding older contents, so over several frames the exemption travels with the data: whatever a later
    command computes from an exempt image is exempt, and an image written whole from images that are not exempt is not exempt any more."""
    exempt = set()
    for body in frames:
        unread = set(unread_dispatches(body))
        for i, cmd in enumerate(body):
            tainted = i in unread or any(r in exempt for r in reads(cmd))
            for w in writes(cmd):
                if tainted:
                    exempt.add(w)
                elif isinstance(cmd, B) or whole(cmd):
                    exempt.discard(w)
    return exempt


def fuses_by_structure(body):
    """True if somewhere a blit directly follows the whole-image dispatch that wrote its source and its destination is named nowhere else
    in the body: whatever else the body holds, that blit can be a second store of the dispatch."""
    for i in range(len(body) - 1):
        d, b = body[i], body[i + 1]
        if isinstance(d, A) and whole(d) and isinstance(b, B) and b.src == d.dst and b.dst != b.src:
            others = [c for j, c in enumerate(body) if j != i + 1]
            if not any(b.dst in reads(c) + writes(c) for c in others):
                return True
    return False


# ---- inputs ----
def exact_inputs(W, H, seed=0):
    """(normals, motion, raytraced) on which the a-trous filter is the identity: ids (x mod 9) + 9 (y mod 9), normals (0, 0, 1), no motion."""
    rng = np.random.default_rng([seed, 21])
    ys, xs = np.mgrid[0:H, 0:W]
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = 1.0
    n[..., 3] = xs % 9 + 9 * (ys % 9)
    motion = np.zeros((H, W, 4), np.float32)
    motion[..., 2], motion[..., 3] = 0.1, 0.7
    rt = np.stack([(rng.random((H, W)) < 0.7), rng.integers(0, 3, size=(H, W)) * 0.5], -1)
    f = lambda x: np.asarray(x, np.float32).astype(np.float16).view(np.uint16)          # noqa: E731
    return f(n), f(motion), f(rt)


def live_inputs(W, H, seed=0):
    """(normals, motion, raytraced) on which the kernels do real work: svgf_cases.live_taps surfaces drawn for step 2, motion (1.25, -0.5)."""
    normals, _ = svgf_cases.live_taps(W, H, 2, seed)
    _, motion, rt = synthetic_svgf_inputs(W, H, seed + 1, motion=(1.25, -0.5))
    return normals, motion, rt


def random_pool(W, H, seed, prev_normals=None, ids=False):
    """Every pool image with random finite fp16 content of its own (in [0, 1): luminance, variance and moments as the kernels meet them), so
    that a command skipped or pointed at another image shows.  prev_normals: last frame's normals, where svgf.comp shall reproject.
    ids: the fourth channel of the i-th four-channel storage image is (x mod 9) + 9 (y mod 9) + 81 (i + 1) -- the pool for `exact_inputs`:
    a body may blit such an image into Normals and the filter stays the identity (every tap still has another id than its centre)."""
    rng = np.random.default_rng([seed, 22])
    pool = {name: rng.random((H, W, CHANNELS[name])).astype(np.float16).view(np.uint16) for name in POOL}
    if ids:
        ys, xs = np.mgrid[0:H, 0:W]
        for i, name in enumerate(STORAGE_RGBA):
            # (the other three channels below 0.5: as normals, n . n' stays below 1 and its 128th power finite -- inf x 0 would be NaN)
            pool[name][..., :3] = (0.5 * rng.random((H, W, 3))).astype(np.float16).view(np.uint16)
            pool[name][..., 3] = (xs % 9 + 9 * (ys % 9) + 81 * (i + 1)).astype(np.float16).view(np.uint16)
    if prev_normals is not None:
        pool["prev_normals"] = np.array(prev_normals, np.uint16)
    return pool


def every_tap_is_rejected(normals, step):
    """The interpreter's premise on the normals image a dispatch reads: each of the 24 taps of every pixel, where it lies in the image,
    has another object id (the fourth channel, truncated) than the pixel."""
    ids = np.asarray(normals, np.uint16).view(np.float16)[..., 3].astype(np.float32).astype(np.int64)
    H, W = ids.shape
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            if (dx or dy) and abs(oy) < H and abs(ox) < W:
                a = ids[max(0, oy):H + min(0, oy), max(0, ox):W + min(0, ox)]
                b = ids[max(0, -oy):H + min(0, -oy), max(0, -ox):W + min(0, -ox)]
                if (a == b).any():
                    return False
    return True


# ---- the truth ----
def interpret(size, frames, inputs, pool_init, oracle, display_size=None, every_frame=False):
    """The commands of every frame's body, strictly in order, on numpy arrays.  Returns {name: image} for the pool after the last frame;
    every_frame: a list of them, one per frame.  A is an identity copy over the pixels the dispatch covers (see the module's docstring: the
    inputs must be `exact_inputs`); B is an array copy; T is oracle.svgf_temporal on the pixels the dispatch covers.  The moments image has
    a twin: svgf.comp reads one and writes the other, and the name goes to the one written (a partial T leaves the twin's older texels)."""
    W, H = size
    pfd = simple_pfd(W, H)
    if display_size is not None:
        pfd["display_size"] = list(display_size)
        pfd["display_size_inverse"] = [1.0 / display_size[0], 1.0 / display_size[1]]
    img = {name: np.array(pool_init[name], np.uint16) for name in POOL}
    img["Normals"], img["Motion"], img["Raytraced"] = (np.array(x, np.uint16) for x in inputs)
    moments_twin = np.zeros((H, W, 2), np.uint16)
    out = []
    for body in frames:
        check_body(body)
        for cmd in body:
            if isinstance(cmd, B):
                if cmd.src != cmd.dst:
                    img[cmd.dst] = img[cmd.src].copy()
                continue
            cw, ch = covered(cmd, W, H)
            if isinstance(cmd, A):
                assert every_tap_is_rejected(img["Normals"], cmd.step), f"{cmd}: the filter is not the identity on these normals"
                img[cmd.dst][:ch, :cw] = img[cmd.src][:ch, :cw]
            else:
                integrated, moments = oracle.svgf_temporal(pfd, *(img[n] for n in T_READS))
                img["a"][:ch, :cw] = integrated[:ch, :cw]
                moments_twin[:ch, :cw] = moments[:ch, :cw]
                img["moments"], moments_twin = moments_twin, img["moments"]
        out.append({name: img[name].copy() for name in POOL})
    return out if every_frame else out[-1]


# ---- the library ----
class DeviceRunner:
    """One context (GpuSvgfHarness with the whole pool) under one set of options, reused for body after body: run() uploads the pool again.
    options: {name: value} for vhr_set_option, set before the graph is built; a name left out keeps the library's default."""

    def __init__(self, size, options=None, display_size=None):
        self.W, self.H = size
        self.frame_body = None
        self.h = GpuSvgfHarness(self.W, self.H, self._record, options=options)
        F4, F2 = abi.FORMAT_R16G16B16A16_SFLOAT, abi.FORMAT_R16G16_SFLOAT
        self.h.alloc_images(c=F4, s=F4, m2=F2)
        self.pfd = simple_pfd(self.W, self.H)
        if display_size is not None:
            self.pfd["display_size"] = list(display_size)
            self.pfd["display_size_inverse"] = [1.0 / display_size[0], 1.0 / display_size[1]]
        self.h.ctx.set_kernel_timing(KERNEL_KINDS)

    def _id(self, name):
        return self.h.images[name]

    def _record(self, ec):
        W, H = self.W, self.H
        for cmd in self.frame_body:
            if isinstance(cmd, B):
                if cmd.src in TRANSIENTS:
                    ec.blit_image_transient_to_storage(TRANSIENTS[cmd.src], self._id(cmd.dst))
                elif cmd.dst in TRANSIENTS:
                    ec.blit_image_storage_to_transient(self._id(cmd.src), TRANSIENTS[cmd.dst])
                else:
                    ec.blit_image_storage_to_storage(self._id(cmd.src), self._id(cmd.dst))
                continue
            xg = groups(W) if cmd.x_groups is None else cmd.x_groups
            yg = groups(H) if cmd.y_groups is None else cmd.y_groups
            if isinstance(cmd, T):
                ec.dispatch(lib.SVGF_SHADER, xg, yg, 1, self.h.push_constants())
            else:
                pc = self.h.push_constants(cmd.step)
                pc["integrated_shadow_and_ao"] = [self._id(cmd.src), self._id(cmd.dst)]
                ec.dispatch(lib.ATROUS_SHADER, xg, yg, 1, pc)

    def _download(self):
        c = self.h.ctx
        return {name: c.download(lib.DENOISED if name == "Denoised" else self._id(name)) for name in POOL}

    def run(self, frames, inputs, pool_init, sync_between_frames=False):
        """-> (pool after the last frame, [pool after every frame] or None, {kernel kind: launches})."""
        c = self.h.ctx
        for body in frames:
            check_body(body)
        for name in POOL:
            c.upload(lib.DENOISED if name == "Denoised" else self._id(name), np.ascontiguousarray(pool_init[name], np.uint16))
        for kind in KERNEL_KINDS:
            c.kernel_time(kind, reset=True)
        per_frame = [] if sync_between_frames else None
        for f, body in enumerate(frames):
            self.frame_body = body
            # the G-buffer is uploaded once: an upload waits for every stream of the context, the side stream's pending dispatch included
            self.h.run(self.pfd, inputs if f == 0 else None, sync=sync_between_frames)
            if sync_between_frames:
                per_frame.append(self._download())
        c.synchronize()
        counts = {kind: int(c.kernel_time(kind)[1]) for kind in KERNEL_KINDS}
        return self._download(), per_frame, counts

    def close(self):
        self.h.close()


def run_device(size, frames, inputs, pool_init, options=None, sync_between_frames=False, display_size=None):
    """One run in a context of its own: see DeviceRunner.run."""
    r = DeviceRunner(size, options, display_size)
    try:
        return r.run(frames, inputs, pool_init, sync_between_frames)
    finally:
        r.close()


# ---- the bodies ----
def reference_body():
    """hybrid_render_path.cpp:291-328 as HybridRenderPath records it: svgf.comp, five a-trous iterations over the ping-pong pair, the first
    one's image into the history, the normals into the previous normals, the fourth one's image into Denoised."""
    body, x, y = [T()], "a", "b"
    for i in range(5):
        body.append(A(x, y, 1 << i))
        if i == 0:
            body.append(B(y, "history"))
        x, y = y, x
    return body + [B("Normals", "prev_normals"), B(y, "Denoised")]


def keeps_ids(frames):
    """True if at every dispatch of the run Normals holds an image that carries ids: the G-buffer of `exact_inputs` or, blitted there, a
    four-channel image of random_pool(ids=True) as the identity filter and the blits have moved it about.  What svgf.comp writes, Motion
    and whatever is computed from them carry none.  (The precondition of `interpret`, from the body alone.)"""
    have = set(STORAGE_RGBA) | {"Normals"}
    for body in frames:
        for cmd in body:
            if isinstance(cmd, T):
                have.discard("a")
            elif isinstance(cmd, A):
                if "Normals" not in have:
                    return False
                if cmd.src not in have:
                    have.discard(cmd.dst)
                elif whole(cmd):
                    have.add(cmd.dst)
            elif cmd.src != cmd.dst:
                (have.add if cmd.src in have else have.discard)(cmd.dst)
    return True


def random_bodies(count=40, seed=20251):
    """`count` bodies of 4 to 9 commands over the pool, each fit to run for two frames on `exact_inputs` (keeps_ids).  After a dispatch, half
    the time the next command blits its output; a blit may go into Normals; half the bodies end in a dispatch nothing reads, and those carry
    a normals blit (without which nothing can go to the side stream): half of them somewhere in front of it, half behind it as the last
    command."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]          # noqa: E731

    def dispatch():
        src = pick(STORAGE_RGBA)
        return A(src, pick([n for n in STORAGE_RGBA if n != src]), pick(STEPS))

    def blit(src=None):
        if src is None:
            r = rng.random()
            if r < 0.15:
                src, dst = pick([("moments", "m2"), ("m2", "moments"), ("Raytraced", "m2")])
                return B(src, dst)
            if r < 0.25:
                return B(pick(STORAGE_RGBA), "Normals")
            src = "Normals" if r < 0.5 else ("Motion" if r < 0.55 else pick(STORAGE_RGBA))
        dsts = [n for n in STORAGE_RGBA if n != src] + ([] if src in TRANSIENTS else ["Denoised"])
        return B(src, "prev_normals" if src == "Normals" and rng.random() < 0.5 else pick(dsts))

    def draw(k):
        n, body = int(rng.integers(4, 10)), []
        while len(body) < n:
            if body and isinstance(body[-1], A) and rng.random() < 0.5:
                body.append(blit(body[-1].dst))
                continue
            r = rng.random()
            body.append(dispatch() if r < 0.5 else (blit() if r < 0.88 else T()))
        if k % 2 == 0:                                           # ends in a dispatch nothing reads, with a copy of the normals in the pass
            last = dispatch()
            copy = B("Normals", pick([x for x in STORAGE_RGBA if x not in (last.src, last.dst)]))
            if k % 4 == 0:
                body[-1] = last
                body[int(rng.integers(1, n - 1))] = copy
            else:
                body[-2:] = [last, copy]
        return body

    bodies = []
    for k in range(count):
        body = draw(k)
        while not keeps_ids([body, body]):
            body = draw(k)
        check_body(body)
        bodies.append(body)
    return bodies


def show(body):
    def one(c):
        if isinstance(c, T):
            return "T" + ("" if whole(c) else f"[{c.x_groups}x{c.y_groups}]")
        if isinstance(c, A):
            return f"A {c.src}>{c.dst}/{c.step}" + ("" if whole(c) else f"[{c.x_groups}x{c.y_groups}]")
        return f"B {c.src}>{c.dst}"
    return "; ".join(one(c) for c in body)
