"""CPU tests of stream.py's host-side helpers (no GPU): the slot header's layout, the names and order of retire()'s tuple, the
"not built with it" guard and the submit / retire loop."""
import collections

import pytest


def test_header_layout_is_the_kernels_layout():
    from articulated_pose_amd.depth import CAM_WORDS, GEOM_WORDS
    from articulated_pose_amd.stream import header_layout
    for B in (1, 4, 32):
        for keyed in (False, True):
            lead = 4 if keyed else 2
            lay = header_layout(B, keyed)
            assert lay.key == slice(0, lead) and lay.seed == slice(0, 2) and lay.base == (slice(2, 3) if keyed else None)
            assert lay.off == slice(lead, lead + B + 1) and lay.nf == slice(lead + B + 1, lead + 2 * B + 1)
            assert lay.geom is None and lay.cam is None and lay.dest is None and lay.words == lead + 2 * B + 1
            d = header_layout(B, keyed, depth=True)
            g0 = lead + 2 * B + 1
            assert (d.key, d.off, d.nf) == (lay.key, lay.off, lay.nf)
            assert d.geom == slice(g0, g0 + GEOM_WORDS * B) and d.cam == slice(d.geom.stop, d.geom.stop + CAM_WORDS * B)
            assert d.dest is None and d.words == d.cam.stop
            i = header_layout(B, keyed, depth=True, label_images=True)
            assert i[:-2] == d[:-2] and i.dest == slice(d.words, d.words + B) and i.words == d.words + B


def test_results_pack_in_the_documented_order_and_unpack_by_name():
    from articulated_pose_amd.stream import RESULT_ORDER, pack_results, unpack_results
    assert RESULT_ORDER == ("tag", "seed", "record", "flags", "articulation", "dense", "label_images", "counts")
    named = {k: k.upper() for k in RESULT_ORDER}
    assert pack_results(named) == ("TAG", "SEED", "RECORD")
    assert pack_results(named, flags=True) == ("TAG", "SEED", "RECORD", "FLAGS")
    assert pack_results(named, articulation=True, dense=True) == ("TAG", "SEED", "RECORD", "ARTICULATION", "DENSE")
    assert pack_results(named, flags=False, label_images=True, counts=True) == ("TAG", "SEED", "RECORD", "LABEL_IMAGES", "COUNTS")
    for asked in (dict(), dict(flags=True), dict(dense=True, flags=True), dict(articulation=True, label_images=True, counts=True)):
        got = unpack_results(pack_results(named, **asked), **asked)
        assert got == {k: named[k] for k in RESULT_ORDER[:3] + tuple(k for k in RESULT_ORDER[3:] if asked.get(k))}


def test_guard_names_the_method_the_class_and_the_option():
    from articulated_pose_amd.stream import check_built_with, only_asked
    owner = collections.namedtuple("Owner", "articulation dense label_images")(False, True, False)
    check_built_with(owner, "retire", "AncshPipeline", articulation=False, dense=True, label_images=False)
    with pytest.raises(RuntimeError) as e:
        check_built_with(owner, "retire", "AncshPipeline", articulation=True, dense=True, label_images=True)      # the first one wins
    assert str(e.value) == "retire(articulation=True) needs AncshPipeline(..., articulation=True)"
    with pytest.raises(RuntimeError) as e:
        check_built_with(owner, "stream_depth_batches", "AncshPipeline", label_images=True)
    assert str(e.value) == "stream_depth_batches(label_images=True) needs AncshPipeline(..., depth_capacity=<pixels>, label_images=True)"
    assert only_asked(articulation=False, dense=True) == {"dense": True} and only_asked(dense=False) == {}


def test_pump_keeps_the_window_full_and_drains_in_order():
    from articulated_pose_amd.stream import pump
    inflight, log = collections.deque(), []

    def submit(k, item):
        assert len(inflight) < 2
        inflight.append(item)
        log.append(("submit", k, item))

    def retire():
        log.append(("retire", inflight[0]))
        return inflight.popleft()
    assert list(pump("abcd", inflight, 2, submit, retire)) == list("abcd") and not inflight
    assert [e[0] for e in log] == ["submit", "submit", "retire", "submit", "retire", "submit", "retire", "retire"]
    assert [e[1] for e in log if e[0] == "submit"] == [0, 1, 2, 3]
    assert list(pump([], inflight, 2, submit, retire)) == []
