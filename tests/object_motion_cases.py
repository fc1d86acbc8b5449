"""What tests/test_object_motion_host.py and tests/test_gpu_object_motion.py share: the contract of "object_motion_vectors" walked on any set of
contexts.  After the i-th successful refit the previous record of every triangle is, bit for bit, the record before that refit -- taken here
from triangle_records() BEFORE the update, and the current records from a fresh context built from the updated arrays, so neither truth comes
from the bookkeeping under test."""
import numpy as np

from tests import partial_refit_cases as cases

SEQUENCE = ("1 one primitive's block", "3 a range over two primitives", "4 two disjoint ranges", "6 one primitive's transform")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def differing_rows(a, b):
    return (bits(a) != bits(b)).any(axis=1)


def apply_to_arrays(vertices, primitives, calls):
    for kind, first, data in calls:
        if kind == "v":
            vertices[first:first + len(data)] = data
        else:
            primitives["transform"][first:first + len(data)] = data


def assert_settled(ctx, what):
    cur, prev = ctx.triangle_records(), ctx.triangle_records(previous=True)
    st = ctx.object_motion_statistics()
    assert same(cur, prev), what
    assert st["active"] == 1 and st["differing_records"] == 0, (what, st)


def walk(scene, contexts, fresh):
    """contexts: [(ctx, refit callable)], all holding `scene` with the option on; fresh(vertices, primitives) -> (n, 9) current records of a
    context built from those arrays.  Returns (vertices, primitives) as they stand after the four updates."""
    vertices, primitives = scene.vertices.copy(), scene.primitives.copy()
    ups = cases.updates(scene)
    moved_last = None
    for name in SEQUENCE:
        truth = contexts[0][0].triangle_records()
        for ctx, _ in contexts:
            assert same(ctx.triangle_records(), truth), name
            cases.apply(ctx, ups[name])
        apply_to_arrays(vertices, primitives, ups[name])
        want = fresh(vertices, primitives)
        moved = differing_rows(truth, want)
        assert 0 < int(moved.sum()) < len(want), name
        for ctx, refit in contexts:
            refit(ctx)
            cur, prev = ctx.triangle_records(), ctx.triangle_records(previous=True)
            assert same(prev, truth), f"{name}: the previous records are not the records before the refit"
            assert same(cur, want), f"{name}: the current records are not a fresh build's"
            st = ctx.object_motion_statistics()
            assert st["active"] == 1 and st["differing_records"] == int(moved.sum()), (name, st)
            if moved_last is not None:                        # moved by the refit before, not by this one: it has stopped
                stopped = moved_last & ~moved
                assert stopped.any() and same(prev[stopped], cur[stopped]), name
        moved_last = moved
    # a refit call with nothing pending: everything has stopped; a second one changes nothing
    for ctx, refit in contexts:
        before = ctx.triangle_records()
        for _ in range(2):
            refit(ctx)
            assert_settled(ctx, "a refit with nothing pending")
            assert same(ctx.triangle_records(), before)
    return vertices, primitives
