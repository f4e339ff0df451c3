"""Which ABI entry ransac_single_batch, ransac_joint_batch and pose_fit_batch (pose/parallel_ancsh_pose.py) call for which arguments,
and where the generator key and the joint-kind array sit in the call: _lib.call is replaced by a recorder, so nothing is launched
and no GPU is needed.  The table below is written out, not derived from the code under test: it is what the wrappers did before
their three argument lists were built in one place each (profiles and tests are keyed by these names)."""
import pytest
import torch

from articulated_pose_amd import _lib
from articulated_pose_amd.pose import parallel_ancsh_pose as PP

SEED, NITER, K = 1234, 8, 2
SINGLE_KEY, JOINT_KEY, FIT_KEYS = 7, 9, (7, 24)       # 0-based positions of the key argument(s) behind the entry's name

# (function, key mode, joint kind given, variant) -> (entry, arguments without the stream)
#   variant, by-value mode only: "plain", "noscalar" (scalar_points=False, ransac_single_batch only), "tie" (a tie window)
TABLE = {
    ("single", "value", False, "plain"): ("ancsh_ransac_single_ex", 15),
    ("single", "value", False, "noscalar"): ("ancsh_ransac_single", 13),
    ("single", "value", False, "tie"): ("ancsh_ransac_single_rec", 19),
    ("single", "dseed", False, "plain"): ("ancsh_ransac_single_rec_dseed", 19),
    ("single", "dkey", False, "plain"): ("ancsh_ransac_single_rec_dkey", 19),
    ("joint", "value", False, "plain"): ("ancsh_ransac_joint_ex", 19),
    ("joint", "value", False, "tie"): ("ancsh_ransac_joint_rec", 23),
    ("joint", "value", True, "plain"): ("ancsh_ransac_joint_rec_kind", 24),
    ("joint", "value", True, "tie"): ("ancsh_ransac_joint_rec_kind", 24),
    ("joint", "dseed", False, "plain"): ("ancsh_ransac_joint_rec_dseed", 23),
    ("joint", "dseed", True, "plain"): ("ancsh_ransac_joint_rec_dseed_kind", 24),
    ("joint", "dkey", False, "plain"): ("ancsh_ransac_joint_rec_dkey", 23),
    ("joint", "dkey", True, "plain"): ("ancsh_ransac_joint_rec_dkey_kind", 24),
    ("fit", "value", False, "plain"): ("ancsh_pose_fit_rec", 37),
    ("fit", "value", False, "tie"): ("ancsh_pose_fit_rec", 37),
    ("fit", "value", True, "plain"): ("ancsh_pose_fit_rec_kind", 38),
    ("fit", "value", True, "tie"): ("ancsh_pose_fit_rec_kind", 38),
    ("fit", "dseed", False, "plain"): ("ancsh_pose_fit_rec_dseed", 37),
    ("fit", "dseed", True, "plain"): ("ancsh_pose_fit_rec_dseed_kind", 38),
    ("fit", "dkey", False, "plain"): ("ancsh_pose_fit_rec_dkey", 37),
    ("fit", "dkey", True, "plain"): ("ancsh_pose_fit_rec_dkey_kind", 38),
}


@pytest.fixture()
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: rec.append((name, args)))
    return rec


@pytest.mark.parametrize("case", sorted(TABLE), ids=lambda c: "-".join([c[0], c[1], "kind" if c[2] else "nokind", c[3]]))
def test_entry_and_key_position(calls, case):
    fn, mode, kind, variant = case
    g = torch.Generator().manual_seed(0)
    off = torch.tensor([0, 5, 9], dtype=torch.int32)                  # two parts of 5 and 4 rows
    src, tgt = torch.rand((9, 3), generator=g), torch.rand((9, 3), generator=g)
    rng0, rng1 = torch.tensor([[0, 5]], dtype=torch.int32), torch.tensor([[5, 9]], dtype=torch.int32)      # one joint
    joint_dir = torch.tensor([[0.0, 0.0, 1.0]])
    seed_dev = torch.tensor([SEED], dtype=torch.int64)
    key_dev = torch.tensor([SEED, 0, 0, 0], dtype=torch.int32)
    joint_kind = torch.tensor([1], dtype=torch.int32) if kind else None
    kw = dict(seed=SEED)
    if mode == "dseed":
        kw.update(seed_dev=seed_dev)
    if mode == "dkey":
        kw.update(key_dev=key_dev, K=K)
    if variant == "tie":
        kw.update(tie_window=PP.TIE_WINDOW)
    if variant == "noscalar":
        kw.update(scalar_points=False)
    if fn == "single":
        PP.ransac_single_batch(off, src, tgt, 0.1, NITER, **kw)
        positions = (SINGLE_KEY,)
    elif fn == "joint":
        PP.ransac_joint_batch(rng0, rng1, src, tgt, joint_dir, 0.1, NITER, joint_kind=joint_kind, **kw)
        positions = (JOINT_KEY,)
    else:
        PP.pose_fit_batch(off, rng0, rng1, src, tgt, joint_dir, 0.1, NITER, NITER, joint_kind=joint_kind, **kw)
        positions = FIT_KEYS
    assert len(calls) == 1
    name, args = calls[0]
    want_name, want_nargs = TABLE[case]
    assert name == want_name
    assert len(args) == want_nargs == len(_lib.SIGNATURES[name]) - 1          # the stream is _lib.call's to add
    # by value: the key itself -- stage B's is the caller's to derive for ransac_joint_batch, seed + 1 for the whole fit
    by_value = (SEED,) if fn != "fit" else (SEED, SEED + 1)
    want_keys = {"value": by_value, "dseed": (seed_dev.data_ptr(),) * len(positions), "dkey": (key_dev.data_ptr(),) * len(positions)}[mode]
    assert tuple(args[p] for p in positions) == want_keys
    if kind:
        assert args[-1] == joint_kind.data_ptr()
    else:
        assert not name.endswith("_kind")
