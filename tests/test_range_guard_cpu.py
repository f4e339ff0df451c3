"""F16x2 range guard, host side (no GPU): the guarded ABI entries exist and refuse bad flag arguments before any launch, the pipeline
refuses the guard for any arithmetic but F16x2, and the host-side weight scan draws the line at 65504, f16's largest value."""
import ctypes

import numpy as np
import pytest

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first

GUARDED = ("ancsh_sa_module_fused_f16x2_grouped_guarded", "ancsh_sa_module_fused_partial_f16x2_grouped_guarded",
           "ancsh_mlp_chain_grouped_fp_f16x2_guarded", "ancsh_sa3_chain_grouped_f16x2_guarded", "ancsh_fp1_chain_grouped_f16x2_guarded",
           "ancsh_fp2_chain_grouped_f16x2_guarded")


def _calls(L, flags, bit0, ngroups=2):
    """every guarded entry point with plausible shapes, non-null (never read) data pointers and the given flag arguments"""
    return {
        "ancsh_sa_module_fused_f16x2_grouped_guarded":
            lambda: L.ancsh_sa_module_fused_f16x2_grouped_guarded(ngroups, 2, 1024, 512, 64, 0, 64, 64, 128, P8, None, P8, P8, P8, P8, flags, bit0, None),
        "ancsh_sa_module_fused_partial_f16x2_grouped_guarded":
            lambda: L.ancsh_sa_module_fused_partial_f16x2_grouped_guarded(ngroups, 2, 512, 128, 64, 128, 128, 256, P8, P8, P8, P8, P8, P8, flags, bit0, None),
        "ancsh_mlp_chain_grouped_fp_f16x2_guarded":
            lambda: L.ancsh_mlp_chain_grouped_fp_f16x2_guarded(ngroups, 2, 1024, 512, 128, P8, P8, P8, P8, P8, P8, P8, flags, bit0, None),
        "ancsh_sa3_chain_grouped_f16x2_guarded":
            lambda: L.ancsh_sa3_chain_grouped_f16x2_guarded(ngroups, 2, 128, 256, 256, 512, 1024, P8, P8, P8, P8, flags, bit0, None),
        "ancsh_fp1_chain_grouped_f16x2_guarded":
            lambda: L.ancsh_fp1_chain_grouped_f16x2_guarded(ngroups, 2, 128, 256, 256, 256, P8, P8, P8, P8, flags, bit0, None),
        "ancsh_fp2_chain_grouped_f16x2_guarded":
            lambda: L.ancsh_fp2_chain_grouped_f16x2_guarded(ngroups, 2, 128, 512, 256, 128, 256, 128, P8, P8, P8, P8, P8, P8, flags, bit0, None),
    }


def test_guarded_symbols_and_abi_version():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    assert L.ancsh_abi_version() >= 9
    for name in GUARDED:
        assert name in _lib.SIGNATURES and hasattr(L, name)
        # the guarded form = the unguarded arguments + (unsigned *range_flags, int flag_bit0) before the stream
        base = _lib.SIGNATURES[name[:-len("_guarded")]]
        assert _lib.SIGNATURES[name] == base[:-1] + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]


@pytest.mark.parametrize("name", GUARDED)
def test_guarded_entries_reject_bad_flag_arguments_before_launch(name):
    from articulated_pose_amd import _lib
    L = _lib.lib()
    assert _calls(L, None, 0)[name]() == -1 and b"null range_flags" in L.ancsh_last_error()
    assert _calls(L, P8, 31)[name]() == -1 and b"32 bits" in L.ancsh_last_error()            # bits 31 and 32 of a paired launch
    assert _calls(L, P8, -1)[name]() == -1 and b"32 bits" in L.ancsh_last_error()


def test_range_guard_needs_f16x2():
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.weights import synthetic_weights
    w = synthetic_weights(3)
    for arith in ("f32", "bf16x3", None):
        with pytest.raises(ValueError, match="range_guard"):
            AncshPipeline(3, w, w, 2, 512, "cpu", arithmetic=arith, range_guard=True)


def _nets(w):
    from articulated_pose_amd.network import Network
    return [("ancsh", Network(3, w, "ancsh", "cpu")), ("npcs", Network(3, w, "npcs", "cpu"))]


def test_weight_scan_draws_the_line_at_f16_max():
    from articulated_pose_amd.pipeline import f16x2_weight_violations
    from articulated_pose_amd.weights import synthetic_weights
    w = synthetic_weights(3)
    assert f16x2_weight_violations(_nets(w)) == []
    name = "SPFN/est_net/layer3/conv1/weights"
    w[name] = np.array(w[name], copy=True)
    w[name].reshape(-1)[17] = 65504.0
    assert f16x2_weight_violations(_nets(w)) == []
    w[name].reshape(-1)[17] = np.nextafter(np.float32(65504.0), np.float32(np.inf))       # 65504.004
    assert [n for n, _ in f16x2_weight_violations(_nets(w))] == ["ancsh:SPFN/est_net/layer3/conv1", "npcs:SPFN/est_net/layer3/conv1"]
    w[name].reshape(-1)[17] = -65505.0
    assert len(f16x2_weight_violations(_nets(w))) == 2
    w[name].reshape(-1)[17] = np.nan                                                              # NaN is not a range violation
    assert f16x2_weight_violations(_nets(w)) == []


def test_weight_scan_skips_the_rows_that_stay_f32():
    """layer2/conv0's feature rows (3..) and fa_layer1/conv_0's rows ..1023 are f32 partial sums on the F16x2 path: not scanned."""
    from articulated_pose_amd.pipeline import f16x2_weight_violations
    from articulated_pose_amd.weights import synthetic_weights
    w = synthetic_weights(3)
    for name, row, flags in (("SPFN/est_net/layer2/conv0/weights", 3, False), ("SPFN/est_net/layer2/conv0/weights", 2, True),
                             ("SPFN/est_net/fa_layer1/conv_0/weights", 1023, False), ("SPFN/est_net/fa_layer1/conv_0/weights", 1024, True)):
        ww = dict(w)
        a = np.array(w[name], copy=True)
        a.reshape(-1, a.shape[-1])[row, 5] = 1e6
        ww[name] = a
        assert bool(f16x2_weight_violations(_nets(ww))) == flags, (name, row)


def test_pipeline_refuses_out_of_range_weights_before_touching_the_gpu():
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.weights import synthetic_weights
    w = synthetic_weights(3)
    bad = dict(w)
    name = "SPFN/nocs_net/fc2_0/weights"
    bad[name] = np.array(w[name], copy=True)
    bad[name].reshape(-1)[0] = 65505.0
    with pytest.raises(ValueError, match="fc2_0"):
        AncshPipeline(3, bad, w, 2, 512, "cpu", arithmetic="f16x2", range_guard=True)
