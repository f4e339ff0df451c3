"""CPU: the redzone arena's own arithmetic (tests/redzone.py), on CPU tensors through its cpu=True keyword: for every dtype the host layer
allocates and misalign 0, 4 and 12, what `zeros`, `full`, `ones`, `empty` and their *_like forms return equals the unpatched function's in
dtype, shape, contiguity and value (empty: 0xFF bytes); the body lies where the block says, misalign rounded down to the element size;
`owns` is true for the tensor and its views and false for anything else; one element written through as_strided before or after the body is
reported as BEFORE / PAST; check() returns the block count; the names are torch's own again after an exception, and an outer arena's after
an inner one."""
import numpy as np
import pytest
import torch

import redzone
from redzone import BODY, GUARD, PAD, PATCHED, Arena, RedzoneError, guarded


def _dtypes():
    from articulated_pose_amd.depth import DEPTH_DTYPES, check_depth_dtype
    return [torch.uint8, DEPTH_DTYPES[check_depth_dtype("uint16")][1], torch.int32, torch.int64, torch.float32, torch.float64]


DTYPES = _dtypes()
MISALIGN = [0, 4, 12]
SHAPE = (3, 5, 7)
REAL = {name: getattr(torch, name) for name in PATCHED}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride() and a.is_contiguous() and a.device == b.device \
        and a.numpy().tobytes() == b.numpy().tobytes()


def _block(arena, t):
    """The live block whose body is t's memory."""
    hit = [b for b in arena.blocks if b[0].untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
           and b[1] == t.storage_offset() * t.element_size()]
    assert len(hit) == 1
    return hit[0]


def test_the_depth_dtype_is_the_one_the_front_end_maps_uint16_to():
    assert DTYPES[1] == torch.int16 and len(set(DTYPES)) == 6


@pytest.mark.parametrize("misalign", MISALIGN)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_values_layout_and_owns(dtype, misalign):
    item = torch.empty((), dtype=dtype).element_size()
    like = REAL["zeros"](SHAPE, dtype=torch.float32)
    with guarded(misalign=misalign, cpu=True) as arena:
        assert all(getattr(torch, n) is not REAL[n] for n in PATCHED)
        made = [(torch.zeros(SHAPE, dtype=dtype, device="cpu"), REAL["zeros"](SHAPE, dtype=dtype)),
                (torch.zeros(*SHAPE, dtype=dtype), REAL["zeros"](*SHAPE, dtype=dtype)),
                (torch.ones(list(SHAPE), dtype=dtype), REAL["ones"](SHAPE, dtype=dtype)),
                (torch.full(SHAPE, 7, dtype=dtype, device=torch.device("cpu")), REAL["full"](SHAPE, 7, dtype=dtype)),
                (torch.full((11,), 255 if dtype == torch.uint8 else -7, dtype=dtype), REAL["full"]((11,), 255 if dtype == torch.uint8 else -7, dtype=dtype)),
                (torch.zeros_like(like, dtype=dtype), REAL["zeros_like"](like, dtype=dtype)),
                (torch.ones_like(like, dtype=dtype), REAL["ones_like"](like, dtype=dtype)),
                (torch.full_like(like, 3, dtype=dtype), REAL["full_like"](like, 3, dtype=dtype)),
                (torch.zeros((0, 4), dtype=dtype), REAL["zeros"]((0, 4), dtype=dtype)),
                (torch.zeros((), dtype=dtype), REAL["zeros"]((), dtype=dtype))]
        for k, (got, want) in enumerate(made):
            assert _same(got, want), (k, got, want)
        e = torch.empty(SHAPE, dtype=dtype)
        el = torch.empty_like(like, dtype=dtype)
        for t in (e, el):
            assert t.dtype == dtype and t.shape == SHAPE and t.is_contiguous() and (t.view(torch.uint8) == BODY).all()
        if dtype.is_floating_point:
            assert torch.isnan(e).all()
        elif dtype != torch.uint8:
            assert (e == -1).all()
        assert len(arena.blocks) == len(made) + 2
        # the layout: PAD guard bytes, misalign rounded down to the element size, the body, at least PAD guard bytes
        for t in [m[0] for m in made] + [e, el]:
            raw, off, nbytes, what = _block(arena, t)
            assert off == PAD + (misalign // item) * item and nbytes == t.numel() * item and raw.numel() >= off + nbytes + PAD
            assert (off - PAD) % item == 0 and (raw[:off] == GUARD).all() and (raw[off + nbytes:] == GUARD).all()
            assert t.data_ptr() % item == 0 and str(dtype) in what
            assert arena.owns(t) and arena.owns(t.view(-1)) and (t.numel() < 2 or arena.owns(t.view(-1)[1:]))
            if t.numel() > 1:
                assert arena.owns(t.view(-1)[::2])
                assert not arena.owns(torch.as_strided(t, (t.numel() + 1,), (1,), storage_offset=t.storage_offset()))      # one element past
                assert not arena.owns(torch.as_strided(t, (2,), (1,), storage_offset=t.storage_offset() - 1))             # one element before
        outside = REAL["zeros"](SHAPE, dtype=dtype)
        assert not arena.owns(outside) and not arena.owns(raw) and not arena.owns(None)
        other = Arena(cpu=True)
        assert not other.owns(e) and other.check() == 0
        assert arena.check() == len(made) + 2 and not arena.owns(e) and arena.check() == 0      # check() empties the arena
    assert all(getattr(torch, n) is REAL[n] for n in PATCHED)


@pytest.mark.parametrize("misalign", MISALIGN)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("maker", ["empty", "zeros", "full", "ones"])
def test_one_element_before_or_past_the_body_is_caught(maker, dtype, misalign):
    make = {"empty": lambda: torch.empty((4, 5), dtype=dtype), "zeros": lambda: torch.zeros((4, 5), dtype=dtype),
            "full": lambda: torch.full((4, 5), 9, dtype=dtype), "ones": lambda: torch.ones((4, 5), dtype=dtype)}[maker]
    item = torch.empty((), dtype=dtype).element_size()
    with pytest.raises(RedzoneError, match=r"%d byte\(s\) PAST the buffer overwritten \(first: 0 bytes past its end\)" % item):
        with guarded(misalign=misalign, cpu=True):
            t = make()
            torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() + t.numel()).fill_(0)       # 0 differs from 0xA5 in every byte
    with pytest.raises(RedzoneError, match=r"%d byte\(s\) BEFORE the buffer overwritten \(nearest: 1 bytes before its start\)" % item):
        with guarded(misalign=misalign, cpu=True):
            t = make()
            torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() - 1).fill_(0)
    with guarded(misalign=misalign, cpu=True) as arena:          # every element of the body written, nothing else: clean
        t, u = make(), make()
        t.fill_(5)
        u.view(-1)[-1] = 3
        assert arena.check() == 2
    with pytest.raises(RedzoneError) as both:                    # both sides of two blocks: four findings in one error
        with guarded(misalign=misalign, cpu=True):
            for t in (make(), make()):
                torch.as_strided(t, (t.numel() + 2,), (1,), storage_offset=t.storage_offset() - 1).fill_(0)
    assert str(both.value).count("BEFORE") == 2 and str(both.value).count("PAST") == 2
    assert all(getattr(torch, n) is REAL[n] for n in PATCHED)


def test_names_are_restored_after_an_exception_and_by_a_nested_arena():
    with pytest.raises(KeyError):
        with guarded(cpu=True):
            torch.zeros((3,), dtype=torch.int32)
            raise KeyError("inside")
    assert all(getattr(torch, n) is REAL[n] for n in PATCHED)
    with guarded(cpu=True) as outer:
        mine = {n: getattr(torch, n) for n in PATCHED}
        a = torch.zeros((3,), dtype=torch.int32)
        with guarded(misalign=4, cpu=True) as inner:
            b = torch.full((3,), 2.0, dtype=torch.float64)
            assert inner.owns(b) and not outer.owns(b) and not inner.owns(a) and len(outer.blocks) == 1      # the inner block is not carved twice
            assert inner.check() == 1
        assert all(getattr(torch, n) == mine[n] for n in PATCHED) and outer.owns(a)
        side = Arena(misalign=12, cpu=True)                      # a second arena next to guarded()'s, patched in for some allocations only
        with side.patched():
            s = torch.zeros((5,), dtype=torch.float32)
        assert all(getattr(torch, n) == mine[n] for n in PATCHED) and side.owns(s) and not outer.owns(s) and s.data_ptr() % 16 == 12
        assert side.check() == 1                                 # no check on leaving patched(): the block was still live
        hand = Arena(cpu=True)                                   # an arena built by hand inside guarded(): torch's own empty underneath
        c = hand.empty((2, 2), dtype=torch.float32)
        assert hand.owns(c) and len(outer.blocks) == 1 and hand.check() == 1
        with pytest.raises(RedzoneError, match="PAST"):
            with guarded(cpu=True):
                t = torch.ones((2,), dtype=torch.uint8)
                torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() + 2).fill_(0)
        assert all(getattr(torch, n) == mine[n] for n in PATCHED)
        assert outer.check() == 1
    assert all(getattr(torch, n) is REAL[n] for n in PATCHED)


def test_calls_the_arena_does_not_take_go_to_torch():
    base = REAL["zeros"]((4, 6), dtype=torch.float32)
    with guarded() as arena:                                     # cpu=False: a CPU tensor, or one without a device, is torch's own
        a, b = torch.zeros((3,), dtype=torch.int32), torch.full((3,), 5, dtype=torch.int64, device="cpu")
        c, d = torch.zeros_like(base), torch.empty((2,), dtype=torch.uint8)
        assert not any(arena.owns(t) for t in (a, b, c, d)) and arena.blocks == []
        assert (a == 0).all() and (b == 5).all() and (c == 0).all() and c.shape == base.shape
        assert arena.check() == 0
    with guarded(cpu=True) as arena:
        t = torch.zeros_like(base.t())                           # not contiguous: the strides are preserved by torch, not by the arena
        assert not arena.owns(t) and t.stride() == base.t().stride()
        t = torch.empty((2, 3, 4, 5), dtype=torch.float32, memory_format=torch.channels_last)
        assert not arena.owns(t) and t.is_contiguous(memory_format=torch.channels_last)
        t = torch.zeros((3,), dtype=torch.float32, requires_grad=True)
        assert not arena.owns(t) and t.requires_grad
        out = REAL["empty"]((3,), dtype=torch.float32)
        assert torch.zeros((3,), out=out) is out and not arena.owns(out)
        assert torch.full((2,), 1.5).dtype == torch.get_default_dtype() and torch.full((2,), 3).dtype == torch.int64      # full's inferred dtype
        assert arena.owns(torch.full((2,), 1.5)) and arena.owns(torch.zeros(2, 3)) and torch.zeros(2, 3).dtype == torch.get_default_dtype()
        assert np.array_equal(torch.full((2, 2), True).numpy(), np.ones((2, 2), bool))
    assert redzone._REAL == REAL


# ---- the problems the GPU tests run under guards, held to what a guard test needs (tests/redzone_cases.py) ---------------------------------------
import redzone_cases as RC      # noqa: E402


@pytest.mark.parametrize("K,dtype,shapes", RC.CASES, ids=RC.IDS)
def test_the_guarded_crops_are_odd_end_at_the_capacity_and_show_the_parts(K, dtype, shapes):
    """By the mirrors alone: the crops' pixel counts are no multiple of 4 (so none of 256), the starts are odd with a gap in between, the last
    crop ends exactly at pixel_capacity; every crop shows a part to the camera and in both predicted frames of the perturbed record, and the
    larger crop shows all of them (K = 8: at least six); the pass's mirror uses pixels of every frame, so the kernels' rows are not empty."""
    import refinement_mirror as RF
    from test_refinement_cpu import refine_table
    case = RC.problem(K, dtype, shapes)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = case["prob"]
    assert geom.shape == (RC.B, 5) and [tuple(g[1:3]) for g in geom.tolist()] == list(RC.SHAPES[shapes])
    px = geom[:, 1] * geom[:, 2]
    assert all(p == 1 or (p % 4 and p % 256) for p in px) and (geom[:, 0] % 2 == 1).all() and (geom[:, 3:] % 2 == 1).all()
    assert geom[0, 0] > 0 and geom[1, 0] > geom[0, 0] + px[0] and geom[1, 0] + px[1] == cap
    drawn = RC.predicted_images(case, case["per"])
    for f in range(RC.B):
        seen = set(case["images"][f][case["images"][f] >= 0].tolist())
        assert seen and all(set(drawn[v * RC.B + f][drawn[v * RC.B + f] >= 0].tolist()) & seen for v in range(2)), f
    assert len(set(case["images"][0][case["images"][0] >= 0].tolist())) >= min(K, 6)
    assert np.isfinite(case["rec"]).all() and np.isfinite(case["per"]).all() and not np.array_equal(case["rec"], case["per"])
    S, _ = RF.evaluate(mesh, render, scene, rigs, nf, case["per"], geom, frames, refine_table(iters=1, min_pixels=1))
    assert S.shape == (RC.B, K, 2, 32) and all((S[f, :, v, 28] > 0).any() for f in range(RC.B) for v in range(2)), S[..., 28]


@pytest.mark.parametrize("kind", RC.STREAM_KINDS)
@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_the_guarded_pipelines_options_pass_the_host_check_and_turn_everything_on(kind, dtype):
    """stream.check_options on each input kind's keywords: accepted, and every flag the kind can carry is on."""
    from articulated_pose_amd.stream import check_options
    spec = RC.stream_kind(kind, dtype)
    o = check_options(spec["B"], spec["N"], **{k: v for k, v in spec["options"].items() if k not in RC.NOT_CHECKED})
    assert o.range_guard and o.articulation and o.joint_states and o.fit_quality and o.ground_truth
    want = dict(raw=("dense",), depth=("label_images",), annotated=("point_ground_truth", "build_point_gt", "build_gt_pose", "annotated_images", "link_counts", "sensor"))
    every = want["annotated"] + ("render", "posed", "reprojection", "refine", "silhouette", "refine_joints", "refine_coverage")
    on = want.get(kind, every)
    assert all(getattr(o, name) for name in on), [name for name in on if not getattr(o, name)]
    assert o.keyed == (kind == "posed") and (o.depth_dtype == dtype) == (kind != "raw")
