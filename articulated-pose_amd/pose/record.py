"""The streamed record's layout, stated once: the pose record and the column blocks the *_rec launches stack behind it (include/ancsh_hip.h).
Every such launch copies the record so far -- the "carried" row -- bit for bit and writes its own block behind it, so a block's columns
depend on which blocks were built before it.  BLOCKS is that order; a new per-part report is one more row of it.  Host-side arithmetic
on a handful of integers, done when a pipeline is built: nothing here touches a device or runs per step."""
import collections
import functools
import itertools

from . import gt_errors, point_gt, quality, refinement, reprojection

Block = collections.namedtuple("Block", "name option key width columns")      # option: the check_options flag that builds the block;
#                                                                               key: the out[...] name of the record that ends with it

_RT = tuple("R%d%d" % (a, k) for a in range(3) for k in range(3)) + ("s", "tx", "ty", "tz")      # a pose: R row-major | s | t
_both = lambda columns: tuple("baseline_" + c for c in columns) + tuple("nonlinear_" + c for c in columns)
_RESIDUALS = ("inliers", "mean", "rms", "median", "max")      # quality.COL_BASELINE / COL_NONLINEAR + 0..4
_ERRORS = ("rpy_err", "xyz_err", "scale_err", "iou", "rel_rot_err")      # gt_errors.ERR_RPY.. / ERR_NL_RPY..

BLOCKS = (
    Block("pose", None, "record", 26, _both(_RT)),
    Block("fit_quality", "fit_quality", "record_wide", quality.FIT_QUALITY_WIDTH - 26,
          ("points", "consensus_a") + tuple("baseline_" + c for c in _RESIDUALS) + ("score_b",) + tuple("nonlinear_" + c for c in _RESIDUALS)),
    Block("gt_errors", "ground_truth", "record_gt", gt_errors.GT_ERROR_WIDTH, _both(_ERRORS) + ("nonlinear_rel_trans_err", "points")),
    Block("point_gt", "point_ground_truth", "record_point_gt", point_gt.POINT_GT_WIDTH, point_gt.POINT_GT_COLUMNS),
    Block("reprojection", "reprojection", "record_reproj", reprojection.REPROJECTION_WIDTH, reprojection.COLUMN_NAMES),
    Block("refinement", "refine", "record_refined", refinement.REFINE_WIDTH, refinement.COLUMN_NAMES),
)
OPTIONS = tuple(b.option for b in BLOCKS[1:])      # the five flags, in the blocks' order
_BY_NAME = {b.name: b for b in BLOCKS}
assert all(len(b.columns) == b.width and len(set(b.columns)) == b.width for b in BLOCKS)


class RecordLayout(object):
    """Where each block lies in the record of a pipeline built with these flags (RecordLayout.of(opts): with an Options', a pipeline's)."""

    def __init__(self, fit_quality=False, ground_truth=False, point_ground_truth=False, reprojection=False, refine=False):
        on = dict(fit_quality=fit_quality, ground_truth=ground_truth, point_ground_truth=point_ground_truth, reprojection=reprojection,
                  refine=refine)
        self.blocks = tuple(b for b in BLOCKS if b.option is None or on[b.option])
        self.names = tuple(b.name for b in self.blocks)
        self._span, self._carried = {}, {}
        self.width, self.key = 0, None
        for b in self.blocks:
            self._carried[b.name] = (self.key, self.width)      # what the block's launch copies: the record so far
            self._span[b.name] = slice(self.width, self.width + b.width)
            self.width, self.key = self.width + b.width, b.key
        self.columns = tuple(b.name + "." + c for b in self.blocks for c in b.columns)

    @classmethod
    def of(cls, opts):
        return layout_for(*(bool(getattr(opts, name)) for name in OPTIONS))

    def __eq__(self, other):
        return isinstance(other, RecordLayout) and self.names == other.names

    def __hash__(self):
        return hash(self.names)

    def __repr__(self):
        return "RecordLayout(%s: %d columns, out[%r])" % (" | ".join(self.names), self.width, self.key)

    def _block(self, name):
        if name not in _BY_NAME:
            raise ValueError("the record has no block %r: its blocks are %s" % (name, ", ".join(_BY_NAME)))
        if name not in self._span:
            option = _BY_NAME[name].option
            raise ValueError("this record holds no %s block (it holds %s): the pipeline was not built with %s"
                             % (name, ", ".join(self.names), "refine=<pose.refinement.pack_refine(...)>" if option == "refine" else option + "=True"))
        return _BY_NAME[name]

    def span(self, name):
        """The block's absolute columns, a slice."""
        self._block(name)
        return self._span[name]

    def carried(self, name):
        """(key, width) of the record the block's launch copies: out[key] is (B, K, width)."""
        if self._block(name).option is None:
            raise ValueError("the pose block is the fit's own record: no launch carries a row into it")
        return self._carried[name]

    def column(self, name, column_name):
        """The absolute index of one named column of a block."""
        b = self._block(name)
        if column_name not in b.columns:
            raise ValueError("the %s block has no column %r: its columns are %s" % (name, column_name, ", ".join(b.columns)))
        return self._span[name].start + b.columns.index(column_name)

    def check(self, record, what="record"):
        """-> record; ValueError unless its last dimension is this layout's width."""
        if record.shape[-1] != self.width:
            raise ValueError("%s has %d columns, the layout (%s) has %d" % (what, record.shape[-1], " | ".join(self.names), self.width))
        return record

    def block(self, record, name):
        """record[..., span(name)] of a numpy array or a torch tensor of this layout's width: a view."""
        return self.check(record)[..., self.span(name)]


@functools.lru_cache(maxsize=None)
def layout_for(*flags):
    """RecordLayout(*flags), built once per combination: for callers inside a step (PoseSolver.solve)."""
    return RecordLayout(*flags)


@functools.lru_cache(maxsize=None)
def carried_widths(name):
    """Every width the record carried into block `name` can have, over the optional blocks in front of it; the first of them varies fastest."""
    before = OPTIONS[:BLOCKS.index(_BY_NAME[name]) - 1]
    return tuple(RecordLayout(**dict(zip(before, reversed(on)), **{_BY_NAME[name].option: True})).carried(name)[1]
                 for on in itertools.product((False, True), repeat=len(before)))


CARRIED_WIDTHS = carried_widths("point_gt")      # pose.point_gt.CARRIED_WIDTHS is this
