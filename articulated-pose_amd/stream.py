"""What AncshPipeline's streaming half (submit / submit_depth / retire / stream_*) and dist.ShardedPipeline's share, each written once:
the slot header's layout, the label buffers, the table of streamed outputs, the names and order of what retire() returns, the "asked for x
but not built with x" guard, and the submit-when-room / retire-when-full loop.  Host-side plumbing only: nothing here launches a kernel."""
import collections

import numpy as np
import torch

# ---- the slot header ---------------------------------------------------------------------------------------------------------
# [seed (int64 bits) -- keyed: the 16-byte key block (ancsh_stream_key: seed, cloud_base, reserved) -- | offsets (B+1) int32 |
#  norm factors (B) float32 | depth: geom (B x GEOM_WORDS) int32 | cam (B x CAM_WORDS) float32 | label_images: dest (B) int32]
# The kernels read it through the pointers AncshPipeline._sample passes: the order is theirs, not this module's to change.
HeaderLayout = collections.namedtuple("HeaderLayout", "key seed base off nf geom cam dest words")


def header_layout(B, keyed=False, depth=False, label_images=False):
    """The int32 word ranges (slices; None = not in this header) of a slot header for B clouds, and its length `words`."""
    from .depth import CAM_WORDS, GEOM_WORDS
    at = 4 if keyed else 2
    parts = dict(key=slice(0, at), seed=slice(0, 2), base=slice(2, 3) if keyed else None)
    for name, n in (("off", B + 1), ("nf", B), ("geom", GEOM_WORDS * B if depth else 0), ("cam", CAM_WORDS * B if depth else 0),
                    ("dest", B if depth and label_images else 0)):
        parts[name] = slice(at, at + n) if n else None
        at += n
    return HeaderLayout(words=at, **parts)


def label_buffers(capacity, device=None):
    """(labels (capacity,) int32 filled -1, values (capacity, 7) float32 filled NaN): what ancsh_raw_point_labels and
    ancsh_depth_label_images write per raw row / per pixel.  On `device`, or (None) in pinned host memory."""
    from .dataset import DENSE_VALUES
    pair = (torch.full((capacity,), -1, dtype=torch.int32, device=device),
            torch.full((capacity, DENSE_VALUES), float("nan"), dtype=torch.float32, device=device))
    return pair if device is not None else tuple(t.pin_memory() for t in pair)


# ---- the table of streamed outputs ---------------------------------------------------------------------------------------------
# An output's extent for a batch of n_valid clouds in slot sl (padding clouds follow the valid ones in every buffer): leading rows to copy.
def per_cloud(sl, n_valid):
    return n_valid


def per_raw_row(sl, n_valid):          # the batch's own offsets: a slot's staging is rewritten only after it retires
    return int(sl.np_off[n_valid])


def per_pixel(sl, n_valid):            # the batch's own geometry {start h w row0 col0}, likewise
    return int(sum(int(g[1]) * int(g[2]) for g in sl.np_geom[:n_valid]))


# How retire() turns an output's pinned buffers into the value it returns (fresh host arrays) ...
def take_rows(host, sl, n_valid, n):
    return host[0][:n].numpy().copy()


def take_dense(host, sl, n_valid, n):
    return host[0][:n].numpy().copy(), host[1][:n].numpy().copy(), sl.np_off[:n_valid + 1].astype(np.int64)


def take_images(host, sl, n_valid, n):
    from .depth import cut_label_images
    return cut_label_images(host[0].numpy()[:n], host[1].numpy()[:n], [(int(g[1]), int(g[2])) for g in sl.np_geom[:n_valid]])


# ... and how the f32 refit's value replaces the flagged clouds' part of it
def patch_items(value, redo, hit):     # indexed by cloud: array rows, or a list of per-frame images
    for c in hit:
        value[c] = redo[c]


def patch_dense(value, redo, hit):     # (labels, values, offsets): cloud c owns rows [offsets[c], offsets[c+1])
    off = value[2]
    for c in hit:
        a, e = off[c], off[c + 1]
        value[0][a:e], value[1][a:e] = redo[0][a:e], redo[1][a:e]


class Output(object):
    """One streamed output of a slot: where the captured step leaves it on the device, its pinned host twin(s), and how a batch's part
    of it is copied out, returned and patched.  source(sl, f32) -> the device tensors behind slot sl's last replay (the f32 graph's for
    f32=True); make_host() -> their pinned twins, one per tensor; refit: the range guard's f32 graph has its own, with their own twins."""

    def __init__(self, name, source, make_host, refit=False, extent=per_cloud, take=take_rows, patch=patch_items):
        self.name, self.source, self.extent, self.take, self.patch = name, source, extent, take, patch
        self.host = make_host()
        self.host32 = make_host() if refit else None

    def copy_out(self, sl, n_valid, f32=False):
        """Enqueue the batch's device -> pinned copies on the current stream."""
        n = self.extent(sl, n_valid)
        for h, d in zip(self.host32 if f32 else self.host, self.source(sl, f32)):
            h[:n].copy_(d[:n], non_blocking=True)

    def value(self, sl, n_valid, f32=False):
        """The batch's value from the pinned twins (once the copies have completed)."""
        return self.take(self.host32 if f32 else self.host, sl, n_valid, self.extent(sl, n_valid))


# ---- what retire() returns ---------------------------------------------------------------------------------------------------
RESULT_ORDER = ("tag", "seed", "record", "flags", "articulation", "dense", "label_images", "counts")
RESULT_ALWAYS = RESULT_ORDER[:3]
BUILT_WITH = dict(articulation="articulation=True", dense="dense=True", label_images="depth_capacity=<pixels>, label_images=True")


def result_names(**asked):
    """The names of retire()'s tuple, in its order: tag, seed, record, then those of flags / articulation / dense / label_images /
    counts that are asked for (counts: always, on a depth pipeline)."""
    return [k for k in RESULT_ORDER if k in RESULT_ALWAYS or asked.get(k)]


def pack_results(named, **asked):
    return tuple(named[k] for k in result_names(**asked))


def unpack_results(got, **asked):
    """pack_results' inverse: a retired tuple -> {name: value}."""
    return dict(zip(result_names(**asked), got))


def only_asked(**asked):
    """Keywords for a pipeline's retire / stream_batches: only the blocks asked for (a stand-in need not know the others)."""
    return {k: True for k, v in asked.items() if v}


def check_built_with(owner, method, cls, **asked):
    """RuntimeError when `method` is asked for an output that `owner` (a `cls`) was not built with."""
    for name in RESULT_ORDER:
        if asked.get(name) and not getattr(owner, name):
            raise RuntimeError("%s(%s=True) needs %s(..., %s)" % (method, name, cls, BUILT_WITH[name]))


def pump(batches, inflight, window, submit, retire):
    """The streaming loop: submit(k, item) for every item of `batches` while fewer than `window` batches are in `inflight`, retire() the
    oldest first when it is full, and drain at the end; yields what retire() returns, in submission order."""
    for k, item in enumerate(batches):
        if len(inflight) == window:
            yield retire()
        submit(k, item)
    while inflight:
        yield retire()
