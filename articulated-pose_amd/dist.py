"""Multi-GPU layout of the hot path: clouds are independent units through both halves (inference-mode
BN, per-cloud pose fit), so a batch is SHARDED across one-process-per-GPU ranks with no data-path
collective, and ONE gather (RCCL over xGMI; backend "nccl" on ROCm) of fixed-size per-cloud pose
records closes the batch.  The reference has no distributed code at all: its only parallelism is
multiprocessing.Process over contiguous slices (evaluation/pose_multi_process.py:53-67), whose
partition rule is kept here."""
import collections
import os
import socket
import subprocess
import sys

import numpy as np
import torch
import torch.distributed as dist

from .stream import (check_built_with, check_options, check_side_inputs, only_asked, pack_results, pump, refuse_built_frame, refuse_side_inputs,
                     require_side_inputs, split_item, unpack_results)

CHILD_ENV = "ANCSH_LOCAL_RANK_CHILD"      # set in the ranks launch_local_ranks() starts: they must not launch again


ADDR_IN_USE_STATUS = 98                  # exit status of a rank whose rendezvous port was taken (errno EADDRINUSE): the launcher retries


def free_port():
    """A port that was free a moment ago.  Closing the probe socket and binding it again in rank 0 is a race; a rank that loses it
    exits with ADDR_IN_USE_STATUS (init_process_group below) and launch_local_ranks starts over on another port."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def init_process_group(backend, **kw):
    """dist.init_process_group for a rank started by launch_local_ranks: a rendezvous port that is already bound ends the rank
    with ADDR_IN_USE_STATUS instead of a traceback, which tells the launcher to retry on a fresh port."""
    try:
        dist.init_process_group(backend, **kw)
    except Exception as e:      # torch raises DistNetworkError / RuntimeError depending on where the bind fails
        msg = str(e)
        if os.environ.get(CHILD_ENV) == "1" and ("EADDRINUSE" in msg or "address already in use" in msg.lower()):
            print("rank %s: rendezvous port %s is in use" % (os.environ.get("RANK"), os.environ.get("MASTER_PORT")), file=sys.stderr, flush=True)
            sys.exit(ADDR_IN_USE_STATUS)
        raise


def init_groups(backend, device=None, probe_timeout_s=180.0, precheck=True):
    """Process groups of one rank: the CONTROL plane (barrier, max over ranks, rank identities) always on gloo, the DATA plane
    (the record gather) on RCCL (`backend` "nccl") when RCCL works on EVERY rank -- decided together: each rank creates the RCCL
    group and runs one probe all_reduce on `device`, the ranks then agree over gloo (MIN of their flags), so either all of them
    gather over RCCL or all of them stage the gather through host memory.  A node whose RCCL cannot start (no usable IPC between
    the processes, two ranks on one GPU, ...) therefore still completes the job and SAYS so.
    What can be known WITHOUT calling RCCL (a rank without a GPU, two ranks on one GPU: rccl_preconditions) is agreed first, so
    those cases never reach the probe.  Beyond that the agreement covers probes that FAIL WITH AN EXCEPTION on the ranks they fail
    on; a probe that fails on one rank by hanging leaves the healthy ranks inside new_group / all_reduce until `probe_timeout_s`,
    after which RCCL's watchdog may end those processes instead of raising: the job then dies (loudly) rather than falls back.
    Returns (data_group or None, note): None = gather on the default gloo group (RecordGatherer stages through the host)."""
    init_process_group("gloo")
    world = dist.get_world_size()
    if backend != "nccl":
        return None, "gloo (host-staged), as requested"
    import datetime
    # Cheap preconditions first, agreed over gloo BEFORE any rank touches RCCL: a probe that fails on one rank only would leave the
    # healthy ranks blocked inside new_group / all_reduce until RCCL's watchdog tears them down (no Python exception to catch), so
    # whatever can be known without RCCL is checked here, on every rank, from the same gathered list.
    why = rccl_preconditions(all_rank_identities(device), os.environ.get("ANCSH_SHARED_GPU_PROBE") == "1") if precheck else ""
    if why:
        return None, "gloo (host-staged): RCCL not attempted (%s)" % why
    ok, err, g = 1, "", None
    try:
        kw = dict(backend="nccl", timeout=datetime.timedelta(seconds=probe_timeout_s))
        try:
            g = dist.new_group(device_id=torch.device(device), **kw)
        except TypeError:                      # a torch whose new_group has no device_id
            g = dist.new_group(**kw)
        t = torch.ones(1, device=device)
        dist.all_reduce(t, group=g)
        if int(t.item()) != world:
            ok, err = 0, "probe all_reduce over %d ranks returned %r" % (world, t.item())
    except Exception as e:                     # DistBackendError / RuntimeError: whatever the backend raises when it cannot start
        ok, err = 0, "%s: %s" % (type(e).__name__, " ".join(str(e).split())[:240])
    flag = torch.tensor([ok], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag.item()) == 1:
        return g, "RCCL"
    errs = [None] * world
    dist.all_gather_object(errs, err)
    bad = ["rank %d: %s" % (r, e) for r, e in enumerate(errs) if e]
    return None, "gloo (host-staged): the RCCL probe failed (%s)" % "; ".join(bad[:2])


def rccl_preconditions(identities, allow_shared=False):
    """Why RCCL cannot carry the gather between these ranks, from their gathered rank_identity() records alone ('' = nothing known
    against it): a rank without a GPU, or two ranks on the same physical GPU (RCCL needs one per rank).  Every rank evaluates the
    same list, so all of them reach the same decision without a collective that could hang."""
    if any(i.get("device_index") is None for i in identities):
        return "rank(s) %s have no GPU" % [i["rank"] for i in identities if i.get("device_index") is None]
    if allow_shared:
        return ""
    seen = {}
    for i in identities:
        key = i.get("pci_bus_id") or i.get("device_uuid") or ("index", i.get("device_index"))
        if key in seen:
            return "ranks %d and %d share GPU %s" % (seen[key], i["rank"], key if isinstance(key, str) else "index %d" % key[1])
        seen[key] = i["rank"]
    return ""


def rank_environment(rank, world, port, base=None):
    """Environment of local rank `rank` of `world`: what torch.distributed.run would export for one node."""
    env = dict(os.environ if base is None else base)
    env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # the host driver only supports dmabuf IPC; a value the user set is kept
    env[CHILD_ENV] = "1"
    return env


def wants_self_launch(n_ranks, environ=None):
    """True when `--gpus n_ranks` was given to a plain `python script.py` (no launcher exported WORLD_SIZE > 1 and this
    process is not itself a rank started by launch_local_ranks)."""
    environ = os.environ if environ is None else environ
    return n_ranks > 1 and int(environ.get("WORLD_SIZE", "1")) == 1 and environ.get(CHILD_ENV) != "1"


def launch_local_ranks(n_ranks, argv, port=None, timeout=None, attempts=3):
    """Start `n_ranks` copies of `argv` (one process per GPU of this node), rank k with RANK = LOCAL_RANK = k, and wait for all
    of them: the counterpart of the reference's only parallel entry (evaluation/pose_multi_process.py:53-67 -- one Process per
    contiguous slice, start all, join all), with the torch.distributed environment so the ranks can form the RCCL group.
    Rank 0 inherits stdout (its JSON line / report is the launcher's output); the stdout of every other rank goes to the
    launcher's stderr, so a rank's own prints cannot interleave with rank 0's line.  Returns 0 when every rank exited 0; when one
    fails the others are terminated (by PID) and its exit code is returned.  With an automatically chosen port, a rank that found
    the port taken (ADDR_IN_USE_STATUS) makes the launcher start over on another port, `attempts` times at most."""
    auto = port is None
    rc = 0
    for _attempt in range(max(1, attempts)):
        rc = _launch_once(n_ranks, argv, free_port() if auto else port, timeout)
        if not (auto and rc == ADDR_IN_USE_STATUS):
            break
    return rc


def _launch_once(n_ranks, argv, port, timeout):
    procs = [subprocess.Popen(list(argv), env=rank_environment(k, n_ranks, port), stdout=None if k == 0 else sys.stderr)
             for k in range(n_ranks)]
    rc = 0
    try:
        import time
        t0 = time.time()
        alive = set(range(n_ranks))
        while alive:
            for k in sorted(alive):
                r = procs[k].poll()
                if r is None:
                    continue
                alive.discard(k)
                if r != 0 and rc == 0:
                    rc = r
                    print("rank %d exited with status %d: stopping the other ranks" % (k, r), file=sys.stderr, flush=True)
                    for j in alive:
                        procs[j].terminate()
            if timeout is not None and time.time() - t0 > timeout and alive:
                rc = rc or 124
                for j in alive:
                    procs[j].terminate()
                timeout = None
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def rank_identity(device=None):
    """Who this rank is: {rank, local_rank, pid, device_index, device_name, device_uuid, pci_bus_id} (device fields None on CPU)."""
    info = dict(rank=int(os.environ.get("RANK", "0")), local_rank=int(os.environ.get("LOCAL_RANK", "0")), pid=os.getpid(),
                device_index=None, device_name=None, device_uuid=None, pci_bus_id=None)
    if device is not None and torch.device(device).type == "cuda":
        idx = torch.device(device).index
        idx = torch.cuda.current_device() if idx is None else idx
        pr = torch.cuda.get_device_properties(idx)
        info.update(device_index=idx, device_name=pr.name, device_uuid=str(getattr(pr, "uuid", "")) or None)
        bus = [getattr(pr, k, None) for k in ("pci_domain_id", "pci_bus_id", "pci_device_id")]
        if bus[1] is not None:
            info["pci_bus_id"] = "%04x:%02x:%02x" % (bus[0] or 0, bus[1], bus[2] or 0)
    return info


def all_rank_identities(device=None, group=None):
    """[rank_identity of rank 0, 1, ...] on every rank (one all_gather_object): the proof of who took part in a run."""
    me = rank_identity(device)
    if not (dist.is_available() and dist.is_initialized()):
        return [me]
    out = [None] * dist.get_world_size(group)
    dist.all_gather_object(out, me, group=group)
    return out


def shard_range(n_items, world_size, rank):
    """Contiguous slice of rank `rank`, the reference's rule (pose_multi_process.py:55,61):
    num_per = int(n/world) + 1; [num_per*k, min(num_per*(k+1), n))."""
    num_per = int(n_items / world_size) + 1
    s = min(num_per * rank, n_items)
    e = min(num_per * (rank + 1), n_items)
    return s, e


class RecordGatherer(object):
    """The ONE collective of the hot path: a fixed-size gather of per-cloud result records on `dst`.

    Every rank contributes a (n_local, ...) tensor of identical shape; `dst` receives them in rank order, i.e. in global
    cloud order for contiguous shards.  Receive buffers are allocated once per `lane` (a batch in flight: gathers of
    different lanes may overlap), so the steady state allocates nothing.  With the "nccl" backend (= RCCL on ROCm) the
    gather is enqueued on the caller's current HIP stream behind the kernels that produce `local` -- no host
    synchronisation; with "gloo" (CPU tests, or several ranks sharing one GPU) the record is staged through host memory
    after synchronising `stream`."""

    def __init__(self, record_shape, dtype, device, dst=0, group=None):
        self.shape, self.dtype, self.dst, self.group = tuple(record_shape), dtype, dst, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)            # group-local
        # `dst` is a GLOBAL rank (what dist.gather takes); compare it in the group's own numbering
        self.dst_local = dst if group is None else dist.get_group_rank(group, dst)
        self.host_staged = dist.get_backend(group) != "nccl"
        self.device = torch.device("cpu") if self.host_staged else torch.device(device)
        self._lanes = {}

    def buffers(self, lane=0):
        """dst: the `world` receive buffers of a lane (valid once that lane's gather has completed); None elsewhere."""
        if self.rank != self.dst_local:
            return None
        if lane not in self._lanes:
            self._lanes[lane] = [torch.empty(self.shape, dtype=self.dtype, device=self.device) for _ in range(self.world)]
        return self._lanes[lane]

    def gather(self, local, lane=0, stream=None):
        if tuple(local.shape) != self.shape or local.dtype != self.dtype:
            raise ValueError("record must be %s %s, got %s %s" % (self.shape, self.dtype, tuple(local.shape), local.dtype))
        if self.host_staged and local.is_cuda:
            if stream is not None:
                stream.synchronize()
            local = local.cpu()
        bufs = self.buffers(lane)
        dist.gather(local.contiguous(), bufs, dst=self.dst, group=self.group)
        return bufs

    def assembled(self, lane=0):
        """dst: (world * n_local, ...) records in global order."""
        bufs = self.buffers(lane)
        return None if bufs is None else torch.cat(bufs, dim=0)


def gather_records(local, n_total, dst=0, group=None):
    """Gather per-cloud records (n_local, ...) of every rank on `dst` in global cloud order.
    Ranks hold shard_range() slices of n_total clouds (ragged: padded to the largest shard so that a
    single fixed-size gather suffices).  Returns the (n_total, ...) tensor on dst, None elsewhere."""
    world = dist.get_world_size(group)
    num_per = int(n_total / world) + 1
    pad = torch.zeros((num_per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[: local.shape[0]] = local
    g = RecordGatherer(pad.shape, pad.dtype, pad.device, dst, group)
    bufs = g.gather(pad)
    if bufs is None:
        return None
    parts = []
    for r in range(world):
        s, e = shard_range(n_total, world, r)
        parts.append(bufs[r][: e - s])
    return torch.cat(parts, dim=0).to(local.device)      # a host-staged (gloo) gather of device records goes back to their device


def balanced_range(n_items, world_size, rank):
    """Contiguous slice of rank `rank` for an IN-MEMORY batch: shard sizes differ by at most one (64 over 4 -> 16,16,16,16; the
    reference's file-slicing rule shard_range() gives 17,17,17,13, and a step is as slow as its largest shard).  shard_range stays
    the rule wherever sub-pickle names depend on it (pose_multi_process.py)."""
    q, r = divmod(n_items, world_size)
    s = rank * q + min(rank, r)
    return s, s + q + (1 if rank < r else 0)


class _NoStream(object):
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _on(stream):
    return _NoStream() if stream is None else torch.cuda.stream(stream)


class ShardedPipeline(object):
    """The north star's multi-GPU composition as ONE callable object: a global batch of depth clouds is split into balanced
    contiguous shards over one-process-per-GPU ranks, every rank runs its shard through its own AncshPipeline (both networks + the
    pose fit, no data-path collective), and ONE gather of the fixed-size (n, K, 26) f64 pose records on `dst` closes each batch --
    issued on the batch's own HIP stream behind the finish kernels (RCCL over xGMI), or staged through the host when the data
    group is gloo.  Counterpart of evaluation/pose_multi_process.py:53-67 (contiguous slices, one worker each, results joined).

    Without an initialised process group (or world 1) it is a plain AncshPipeline whose records() are the local ones.
    `pipeline_factory(num_parts, weights_ancsh, weights_npcs, n_local, num_points, device, slots=..., **kw)` builds the per-rank
    pipeline (default AncshPipeline; the gloo CPU tests inject a stand-in with the same step()/slot interface).

    raw_capacity (rows PER RANK): the streaming entry -- submit() / retire() / stream_batches() of raw clouds, every rank iterating the
    same global batches.  The per-rank pipeline is then built with raw_capacity and keyed=True, and each rank submits its shard with
    cloud_base = lo, so a cloud is sampled and fitted as its global index whatever the world size (include/ancsh_hip.h,
    ancsh_stream_key); its records are gathered on `dst` over the gloo control group (the default group init_groups creates).
    articulation=True (with raw_capacity only): the stream also yields the (n_valid, K, 12) articulation blocks, packed with the records
    into the same gather; step() / records() over RCCL do not carry them.
    dense=True (with raw_capacity only): the stream also yields every raw row's (labels, values, offsets) (AncshPipeline(dense=True)),
    gathered on dst in global cloud order by one more padded gather per batch.
    joint_source ("gt" | "predicted"): passed to every rank's pipeline (AncshPipeline(joint_source=...)).  "predicted": solve(P, None,
    pred) and load_inputs(P, None, pred) need no labels, and the raw stream takes (n_raw, 3) xyz clouds (or (n_raw, 4), 4th column
    ignored) through the keyed xyz sampler.
    joint_types (None | "revolute" | "prismatic" | K - 1 of them): passed to every rank's pipeline (AncshPipeline(joint_types=...)); the
    kind array repeats per cloud, so a shard's slice of it is the shard's own array and sharded streams stay byte-equal to one GPU's.
    joint_states=True (with articulation=True): the blocks are the (n_valid, K, 20) ones (AncshPipeline(joint_states=True)), gathered with
    the records in the same single gather.
    The streamed record's blocks (pose.record.BLOCKS; self.record_layout says where each lies, as every rank's pipeline.record_layout does)
    travel in that single gather, [record | articulation block] a row, and dst returns the whole record:
    fit_quality=True (with raw_capacity only): every rank's pipeline is built with it (AncshPipeline(fit_quality=True)): the fit-quality block.
    ground_truth=True (with raw_capacity only): every rank's pipeline is built with ground_truth=True and submit() hands it its shard's rows
    of the batch's (n_valid, K, 19) ground truth: the error block (ancsh_gt_error_rec).
    point_ground_truth=True (with raw_capacity and articulation=True): every rank's pipeline is built with point_ground_truth=True, takes
    its shard's (n_raw, 18) clouds and gets its shard's rows of the batch's (n_valid, 13) frames from submit(): the point-gt block
    (ancsh_point_gt_rec).
    build_point_gt=True (with point_ground_truth=True): every rank's pipeline builds its rows on the device (AncshPipeline(build_point_gt=
    True)) from its shard's (n_raw, 7) annotated clouds and its shard's rows of the batch's (n_valid, RIG_WIDTH) rigs, handed out as the
    frames are.
    build_gt_pose=True (with point_ground_truth=True): every rank's pipeline fits its shard's ground-truth poses on the device
    (AncshPipeline(build_gt_pose=True)): submit() takes no frame, and every rank still gets its shard's rows of gt, for the box extents."""

    def __init__(self, num_parts, weights_ancsh, weights_npcs, global_batch, num_points, device="cuda:0", data_group=None, dst=0,
                 slots=1, pipeline_factory=None, gather_single=False, raw_capacity=None, articulation=False, dense=False, joint_source="gt",
                 joint_types=None, joint_states=False, fit_quality=False, ground_truth=False, point_ground_truth=False, build_point_gt=False,
                 build_gt_pose=False, **pipeline_kw):
        from .pose.parallel_ancsh_pose import check_joint_types
        check_joint_types(joint_types, num_parts)      # before anything touches a GPU or a process group
        if pipeline_kw.get("depth_capacity") is not None:
            raise ValueError("ShardedPipeline does not shard the depth front end (depth_capacity): stream depth frames through "
                             "AncshPipeline.submit_depth on one GPU")
        if pipeline_kw.get("reprojection"):
            raise ValueError("ShardedPipeline does not shard rendered frames: reprojection=True re-renders the mesh of a pipeline built with "
                             "render_mesh=<depth.pack_mesh(...)>, which AncshPipeline takes on one GPU (submit_render / submit_posed)")
        if pipeline_kw.get("refine") is not None:
            raise ValueError("ShardedPipeline does not shard rendered frames: refine=<pose.refinement.pack_refine(...)> re-renders the mesh of a "
                             "pipeline built with render_mesh=<depth.pack_mesh(...)>, which AncshPipeline takes on one GPU (submit_render / "
                             "submit_posed)")
        if pipeline_kw.get("joint_values"):
            raise ValueError("ShardedPipeline does not shard rendered frames: joint_values=True reads the joint values off the part poses of a "
                             "pipeline built with kinematics=<depth.pack_kinematics(...)>, which AncshPipeline takes on one GPU (submit_posed)")
        # what only the raw stream carries (step() / records(), the RCCL path, keep the 26-column record), then the rules shared with
        # AncshPipeline.  The articulation block travels with the records in the SAME gather -- one (n_max, K, record_width + art_width)
        # float64 row per rank, split on dst --, the ground truth, frames and rigs are handed out by submit(), shard by shard.
        for name, asked in (("articulation", articulation), ("fit_quality", fit_quality), ("ground_truth", ground_truth)):
            if asked and raw_capacity is None:
                raise ValueError("%s=True is carried by the raw stream only (submit / retire / stream_batches): it needs raw_capacity" % name)
        self.opts = o = check_options(global_batch, None, True, pipeline_kw.get("inlier_th", 0.1), raw_capacity, keyed=raw_capacity is not None,
                                      articulation=articulation, joint_states=joint_states, fit_quality=fit_quality, ground_truth=ground_truth,
                                      point_ground_truth=point_ground_truth, build_point_gt=build_point_gt, joint_source=joint_source,
                                      build_gt_pose=build_gt_pose)
        if dense and raw_capacity is None:
            raise ValueError("dense=True labels the raw rows of the stream (submit / retire / stream_batches): it needs raw_capacity")
        self.dense, self.joint_source, self.record_width, self.art_width = bool(dense), joint_source, o.record_width, o.art_width
        self.record_layout = o.layout           # where each block of the streamed record lies (pose.record.RecordLayout), as every rank's pipeline has it
        self.couple = bool(pipeline_kw.get("couple", True))
        # only what differs from the default is passed on: a per-rank stand-in built before an option need not know it
        given = dict(joint_types=joint_types, joint_source=None if joint_source == "gt" else joint_source, dense=self.dense)
        for name in ("articulation", "joint_states", "fit_quality", "ground_truth", "point_ground_truth", "build_point_gt", "build_gt_pose"):
            setattr(self, name, getattr(o, name))
            given[name] = getattr(o, name)
        pipeline_kw.update({k: v for k, v in given.items() if v})
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size() if self.distributed else 1
        self.rank = dist.get_rank() if self.distributed else 0
        if global_batch < self.world:
            raise ValueError("global_batch %d < %d ranks: a rank would hold no cloud" % (global_batch, self.world))
        self.K, self.global_batch, self.dst = num_parts, global_batch, dst
        self.lo, self.hi = balanced_range(global_batch, self.world, self.rank)
        self.n_local, self.n_max = self.hi - self.lo, -(-global_batch // self.world)
        self.ragged = global_batch % self.world != 0
        if pipeline_factory is None:
            from .pipeline import AncshPipeline as pipeline_factory
        self.raw_capacity = None if raw_capacity is None else int(raw_capacity)
        if self.raw_capacity is not None:
            pipeline_kw.update(raw_capacity=self.raw_capacity, keyed=True)
            if self.world > 1 and "gloo" not in str(dist.get_backend()):
                raise ValueError("stream_batches gathers host records over the default process group, which must be gloo (dist.init_groups "
                                 "creates it); got %r" % dist.get_backend())
        self.seed = int(pipeline_kw.get("seed", 0))      # batch k of a stream: seed + 2k on every rank (AncshPipeline's default is 0)
        self.pipe = pipeline_factory(num_parts, weights_ancsh, weights_npcs, self.n_local, num_points, device, slots=slots, **pipeline_kw)
        self.gatherer = RecordGatherer((self.n_max, num_parts, 26), torch.float64, device, dst, data_group) \
            if self.world > 1 or (gather_single and self.distributed) else None      # gather_single: run the collective even with one rank
        # a host-staged gather blocks the host on the batch it gathers: done for the batch just issued it would leave ONE batch in
        # flight, so a slot's record is gathered right before the slot is reused (its batch finished long ago); flush() drains
        self.lagged = self.gatherer is not None and self.gatherer.host_staged
        self._pending, self._pad = [], {}
        self._stream = collections.deque()       # streaming: (tag, seed, n_valid, submitted here, raw rows per cloud) of unretired global batches
        self._stream_submitted = 0
        self._stream_bufs = None

    # ---- inputs -------------------------------------------------------------------------------------------------------------
    def load_inputs(self, P, joint_cls=None, pred=None, slot=None, is_global=True):
        """is_global: arrays hold the whole batch (global_batch leading) and this rank takes rows [lo, hi); else they ARE the shard.
        joint_cls: None with joint_source="predicted" (the association is pred['index_per_point'] or the network's own head)."""
        from .pipeline import check_joint_inputs
        check_joint_inputs(self.joint_source, self.couple, joint_cls, pred)
        if is_global:
            if len(P) != self.global_batch:
                raise ValueError("expected %d clouds, got %d" % (self.global_batch, len(P)))
            cut = lambda a: None if a is None else a[self.lo:self.hi]
            P, joint_cls = cut(P), cut(joint_cls)
            pred = None if pred is None else {k: cut(v) for k, v in pred.items()}
        self.pipe.load_inputs(P, joint_cls, pred, slot=slot)

    def load_draws(self, draws_a, draws_b, slot=None, is_global=True):
        if is_global:
            draws_a, draws_b = draws_a[self.lo:self.hi], None if draws_b is None else draws_b[self.lo:self.hi]
        self.pipe.load_draws(draws_a, draws_b, slot=slot)

    def prepare(self):
        self.pipe.prepare()
        return self

    # ---- one batch ----------------------------------------------------------------------------------------------------------
    def _gather(self, sl):
        rec = sl.out["record"]
        if self.ragged:                   # fixed-size collective: shards one cloud short are padded to the largest
            pad = self._pad.get(id(sl))
            if pad is None:
                pad = self._pad[id(sl)] = torch.zeros((self.n_max,) + tuple(rec.shape[1:]), dtype=rec.dtype, device=rec.device)
            with _on(sl.stream):          # ordered behind the kernels that write the record (a host-staged gather synchronises this stream next)
                pad[: rec.shape[0]].copy_(rec)
            rec = pad
        self.gatherer.gather(rec, lane=id(sl), stream=sl.stream)

    def step(self):
        """Issue the next batch of this rank's shard (asynchronous) and its record gather.  Returns (slot, outputs)."""
        if self.lagged:
            nxt = self.pipe.next_slot()
            if nxt in self._pending:
                self._gather(nxt)
                self._pending.remove(nxt)
        sl, out = self.pipe.step()
        if self.gatherer is not None:
            if self.lagged:
                self._pending.append(sl)
            else:
                with _on(sl.stream):
                    self._gather(sl)
        return sl, out

    def flush(self):
        """Complete the gathers a host-staged data group still owes (no-op over RCCL: those are already enqueued)."""
        for sl in self._pending:
            self._gather(sl)
        self._pending = []

    def synchronize(self):
        self.flush()
        self.pipe.synchronize()

    def records(self, slot=None):
        """dst: the (global_batch, K, 26) f64 records of the batch last issued on `slot` (default: the most recent step), in global
        cloud order; None on the other ranks.  Valid after synchronize().  Where the result lives depends on how it was gathered: without a
        gatherer (world 1) it is the slot's own record on the pipeline's device; over RCCL it is on `device` too; with a host-staged
        (gloo) data group -- which init_groups may have fallen back to -- it is a CPU tensor.  (gather_records() moves its result back
        to the records' device; this method does not.)  A caller that needs one place calls .cpu() or .to(device) on it."""
        sl = slot if slot is not None else self.pipe.slots[(self.pipe._next - 1) % len(self.pipe.slots)]
        if self.gatherer is None:
            return sl.out["record"]
        bufs = self.gatherer.buffers(id(sl))
        if bufs is None:
            return None
        parts = []
        for r in range(self.world):
            s, e = balanced_range(self.global_batch, self.world, r)
            parts.append(bufs[r][: e - s])
        return torch.cat(parts, dim=0)

    def solve(self, P, joint_cls=None, pred=None, is_global=True):
        """One global batch end to end: shard, run, gather, wait.  Returns records() (dst) / None (other ranks)."""
        self.load_inputs(P, joint_cls, pred, is_global=is_global)
        if getattr(self.pipe, "slots", None) and getattr(self.pipe.slots[0], "out", None) is None and hasattr(self.pipe, "prepare"):
            self.pipe.prepare()
        self.step()
        self.synchronize()
        return self.records()

    # ---- streaming: raw clouds of global batches in, records gathered on dst (raw_capacity set) --------------------------------------
    def shard_of(self, n_valid, rank=None):
        """[s, e) of the global batch's clouds that rank `rank` (default: this one) serves when the batch holds n_valid clouds: its
        balanced_range over global_batch cut at n_valid (a short batch leaves trailing ranks fewer clouds, or none)."""
        lo, hi = balanced_range(self.global_batch, self.world, self.rank if rank is None else rank)
        return min(lo, n_valid), min(hi, n_valid)

    def _check_batch(self, clouds, norm_factors):
        """The checks of AncshPipeline.submit on EVERY rank's shard, so that every rank raises the same ValueError (before anything is
        enqueued and before any collective) or none does.  -> (clouds, norm factors) as check_raw_clouds returns them."""
        from .dataset import check_stream_key
        clouds, nf = self.opts.rows.check(clouds, norm_factors, self.K, self.global_batch)
        for r in range(self.world):
            s, e = self.shard_of(len(clouds), r)
            if e == s:
                continue
            lo, hi = balanced_range(self.global_batch, self.world, r)
            check_stream_key(lo, hi - lo, self.K)
            rows = sum(c.shape[0] for c in clouds[s:e]) + (hi - lo - (e - s)) * clouds[s].shape[0]      # + padding with its first cloud
            if rows > self.raw_capacity:
                raise ValueError("rank %d's shard of the batch (clouds %d..%d) needs %d raw rows (short shards are padded with their first "
                                 "cloud), raw_capacity is %d per rank" % (r, s, e - 1, rows, self.raw_capacity))
        return clouds, nf

    def submit(self, clouds, norm_factors, tag=None, gt=None, frame=None, rig=None):
        """Enqueue one GLOBAL batch (every rank calls this with the same batch): clouds = 1..global_batch raw (n_raw, 4) arrays, one norm
        factor each.  This rank submits its shard -- nothing when a short batch leaves it no cloud -- to its pipeline with seed
        seed + 2k (k = global batches submitted so far) and cloud_base = lo.  A bad batch raises ValueError on every rank, a full
        in-flight window RuntimeError on every rank; either way nothing is enqueued and the stream stays usable.  gt
        (ShardedPipeline(..., ground_truth=True); ValueError otherwise): the batch's (n_valid, K, 19) ground truth, checked whole on
        every rank; this rank's pipeline gets rows [s, e) of it.  None: a batch without ground truth.  frame
        (ShardedPipeline(..., point_ground_truth=True); ValueError otherwise): the batch's (n_valid, 13) frames, handed out the same
        way.  rig (ShardedPipeline(..., build_point_gt=True), which takes (n_raw, 7) annotated clouds; ValueError otherwise, and when it is
        missing there): the batch's (n_valid, RIG_WIDTH) rigs, handed out the same way.  World 1: the local pipeline's submit."""
        if self.raw_capacity is None:
            raise RuntimeError("submit() needs ShardedPipeline(..., raw_capacity=<rows per rank>)")
        built, given = self.opts.inputs, dict(gt=gt, frame=frame, rig=rig)
        refuse_built_frame(self.opts, frame, "ShardedPipeline")
        refuse_side_inputs(built, given, "ShardedPipeline")
        require_side_inputs(built, given)
        if self.world == 1:
            return self.pipe.submit(clouds, norm_factors, tag=tag, **{inp.name: given[inp.name] for inp in built})
        clouds, nf = self._check_batch(clouds, norm_factors)
        more = check_side_inputs(built, given, len(clouds), self.K, "ShardedPipeline")      # whole, on every rank
        if len(self._stream) == len(self.pipe.slots):
            raise RuntimeError("all %d slots hold unretired batches: retire() one first" % len(self.pipe.slots))
        seed = self.seed + 2 * self._stream_submitted
        s, e = self.shard_of(len(clouds))
        if e > s:
            self.pipe.submit(clouds[s:e], nf[s:e], seed=seed, tag=tag, cloud_base=self.lo,
                             **{name: None if v is None else v[s:e] for name, v in more.items()})
        self._stream.append((tag, seed, len(clouds), e > s, np.array([c.shape[0] for c in clouds], np.int64)))
        self._stream_submitted += 1

    def _gather_dense(self, got, sizes, n_valid):
        """The raw rows of one global batch on dst: every rank pads its shard's rows to the largest shard's count (all ranks know every
        shard's rows: they iterate the same batch) and sends [label | the 7 values' bits] int32 rows in ONE gather.  dst -> (labels (R,) int32,
        values (R, 7) float32, offsets (n_valid+1,) int64) in global cloud order; other ranks -> None."""
        from .dataset import DENSE_VALUES
        cut = [self.shard_of(n_valid, r) for r in range(self.world)]
        counts = [int(sizes[a:b].sum()) for a, b in cut]
        width = 1 + DENSE_VALUES
        buf = np.zeros((max(1, max(counts)), width), np.int32)          # int32 words: the values' bits travel untouched
        if got is not None:
            labels, values, _ = got
            buf[:labels.shape[0], 0] = labels
            buf[:labels.shape[0], 1:] = values.view(np.int32)
        on_dst = self.rank == self.dst
        bufs = [torch.empty(buf.shape, dtype=torch.int32) for _ in range(self.world)] if on_dst else None
        dist.gather(torch.from_numpy(buf), bufs, dst=self.dst)
        if not on_dst:
            return None
        rows = np.concatenate([bufs[r].numpy()[:n] for r, n in enumerate(counts)], axis=0)
        off = np.zeros(n_valid + 1, np.int64)
        np.cumsum(sizes, out=off[1:])
        return np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1:]).view(np.float32), off

    def retire(self, flags=False, articulation=False, dense=False):
        """Wait for the oldest global batch and gather its records on dst (every rank calls this): dst -> (tag, seed, record
        (n_valid, K, 26) float64 in global cloud order), the other ranks -> (tag, seed, None).  flags=True: + the range-guard flag
        words (n_valid,) int32 on dst (None elsewhere).  The gather is one fixed-size (n_max, K, 26) float64 dist.gather over the
        default (gloo) group, padded per rank; every rank derives the valid counts from the split rule, so no count is exchanged.
        articulation=True (ShardedPipeline(..., articulation=True)): + the (n_valid, K, 12) articulation block on dst (None elsewhere) as
        the last element, gathered in the records' gather: each rank packs [record | block] into (n_max, K, record_width + art_width)
        float64 rows (joint_states=True: the (n_valid, K, 20) block; fit_quality, ground_truth, point_ground_truth: the record is the
        self.record_layout.width columns of pose.record.BLOCKS' blocks).
        dense=True (ShardedPipeline(..., dense=True)): + (labels (R,) int32, values (R, 7) float32, offsets (n_valid+1,) int64) of the
        batch's raw rows in global cloud order on dst (None elsewhere), last; one more gather (_gather_dense).
        World 1: the local pipeline's retire()."""
        check_built_with(self, "retire", "ShardedPipeline", articulation=articulation, dense=dense)
        if self.world == 1:
            return self.pipe.retire(flags, **only_asked(articulation=articulation, dense=dense))
        if not self._stream:
            raise RuntimeError("retire(): no batch in flight")
        tag, seed, n_valid, here, sizes = self._stream.popleft()
        s, e = self.shard_of(n_valid)
        rw = self.record_width                                         # the streamed record's columns: self.record_layout.width
        width = rw + self.art_width if self.articulation else rw      # [record | articulation block (12 or 20)]: one gather either way
        rec = np.zeros((self.n_max, self.K, width), np.float64)
        words = np.zeros((self.n_max,), np.int32)
        got = {}
        if here:             # the per-rank pipeline's public retire(), with only the keywords it was built for
            built = dict(articulation=self.articulation, dense=self.dense)
            got = unpack_results(self.pipe.retire(flags, **only_asked(**built)), flags=flags, **built)
            rec[:e - s, :, :rw] = got["record"]
            if self.articulation:
                rec[:e - s, :, rw:] = got["articulation"]
            if flags:
                words[:e - s] = got["flags"]
        on_dst = self.rank == self.dst
        if self._stream_bufs is None and on_dst:
            self._stream_bufs = ([torch.empty((self.n_max, self.K, width), dtype=torch.float64) for _ in range(self.world)],
                                 [torch.empty((self.n_max,), dtype=torch.int32) for _ in range(self.world)])
        bufs = self._stream_bufs if on_dst else (None, None)
        dist.gather(torch.from_numpy(rec), bufs[0], dst=self.dst)
        if flags:
            dist.gather(torch.from_numpy(words), bufs[1], dst=self.dst)
        dn = self._gather_dense(got.get("dense"), sizes, n_valid) if self.dense else None
        out = dict(tag=tag, seed=seed, record=None, flags=None, articulation=None, dense=dn)     # what the other ranks return
        if on_dst:
            cut = [self.shard_of(n_valid, r) for r in range(self.world)]
            packed = np.concatenate([bufs[0][r].numpy()[:b - a] for r, (a, b) in enumerate(cut)], axis=0)
            out["record"] = np.ascontiguousarray(packed[:, :, :rw])
            if flags:
                out["flags"] = np.concatenate([bufs[1][r].numpy()[:b - a] for r, (a, b) in enumerate(cut)], axis=0)
            if articulation:
                out["articulation"] = np.ascontiguousarray(packed[:, :, rw:])
        return pack_results(out, flags=flags, articulation=articulation, dense=dense)

    def stream_batches(self, batches, flags=False, articulation=False, dense=False):
        """Generator over submit / retire of GLOBAL batches (every rank iterates the same batches): batches yields (clouds, norm_factors)
        or (clouds, norm_factors, tag) (tag defaults to the batch's index); up to len(slots) batches stay in flight; yields (tag, seed,
        record) in submission order -- record = the batch's (n_valid, K, 26) records in global cloud order on dst, None on the other
        ranks (flags=True: + the flag words).  The records equal those of one AncshPipeline.stream_batches over the same batches (same
        seed, lm_schedule).  ShardedPipeline(..., ground_truth=True): batches yields (clouds, norm_factors, gt) or (clouds, norm_factors,
        gt, tag), as AncshPipeline.stream_batches; point_ground_truth=True: the frame behind gt, in front of the tag; build_point_gt=True: the rig behind the frame.  articulation=True: + the (n_valid, K, 12) articulation blocks in global cloud order; dense=True: + the raw rows'
        (labels, values, offsets) in global cloud order, last (see retire()).  World 1 (or no process group): the local pipeline's
        stream_batches."""
        check_built_with(self, "stream_batches", "ShardedPipeline", articulation=articulation, dense=dense)
        if self.world == 1:
            yield from self.pipe.stream_batches(batches, flags, **only_asked(articulation=articulation, dense=dense))
            return

        def submit(k, item):
            clouds, norm_factors, side, tag = split_item(item, self.opts.inputs, k)
            self.submit(clouds, norm_factors, tag=tag, **side)
        yield from pump(batches, self._stream, len(self.pipe.slots), submit, lambda: self.retire(flags, articulation, dense))
