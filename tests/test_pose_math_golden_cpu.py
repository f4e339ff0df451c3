"""tests/golden/pose_math.npz is what tests/golden/gen_pose_math_golden.py writes: regenerated here (mpmath at 50 digits, seeded,
a few seconds) and compared with the committed file, so neither the cases nor the bars of test_pose_math_gpu.py can drift from the
recipe.  Arguments and mpmath values must be identical.  The recorded errors of the float64 references come from LAPACK / libm /
scipy builds and may differ in the last bits between machines: they, and the bars derived from them, must agree within a factor of two."""
import importlib.util
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_pose_math_golden_regenerates():
    spec = importlib.util.spec_from_file_location("gen_pose_math_golden", os.path.join(G, "gen_pose_math_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.generate()
    with np.load(os.path.join(G, "pose_math.npz")) as z:
        old = {k: z[k] for k in z.files}
    assert sorted(new) == sorted(old)
    for k in old:
        if k.endswith("_ref") or k.endswith("_bar"):
            assert 0.5 * float(old[k]) <= float(new[k]) <= 2.0 * float(old[k]), k
            if k.endswith("_bar") and k != "recip_ulp_bar":
                ref = float(old[k[:-4] + "_ref"])
                assert float(old[k]) == 64.0 * max(ref, 2.0 ** -52), k                  # the bar is 64 x the reference's error, floor 64 eps
        else:
            assert old[k].shape == new[k].shape and np.array_equal(old[k], new[k]), k
    assert os.path.getsize(os.path.join(G, "pose_math.npz")) < 512 * 1024
