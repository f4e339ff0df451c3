"""Pure-numpy mirror of ancsh_point_gt_build (test infrastructure): the statements of include/ancsh_hip.h on dataset.pack_joint_rig's
table, float64, vectorised over the rows of one cloud.  It lets the GPU tests cover shapes beyond the golden fixture, and the golden
generator read every entry's distance h."""
import numpy as np

ROT, GMAP, HEAD, ENTRY = 4, 13, 22, 9


def part_width(K):
    return 15 + ENTRY * K


def rig_width(K):
    return HEAD + K * part_width(K)


def build_rows(src, rig, K, return_h=False):
    """src (n, 7) float32 [x y z | c | part], rig (rig_width(K),) float64 -> (n, 18) float32 rows (return_h: and a list of (row indices,
    entry k, kind, h) per part and entry)."""
    src = np.asarray(src, np.float32)
    rig = np.asarray(rig, np.float64)
    assert src.ndim == 2 and src.shape[1] == 7 and rig.shape == (rig_width(K),)
    n = src.shape[0]
    out = np.full((n, 18), np.nan, np.float32)
    out[:, :3] = src[:, :3]
    out[:, 3] = out[:, 17] = -1
    thres, default, le, rot = rig[0], rig[1], rig[2] != 0, rig[3] != 0
    R = rig[ROT:ROT + 9].reshape(3, 3)
    lo0, nf0, tail0 = rig[GMAP:GMAP + 3], rig[GMAP + 3:GMAP + 6], rig[GMAP + 6:GMAP + 9]
    part = src[:, 6]
    leads = np.ones(n, bool)
    leads[1:] = part[1:] != part[:-1]
    hs = []
    with np.errstate(all="ignore"):
        for j in range(K):
            idx = np.flatnonzero(part == np.float32(j))
            if idx.size == 0:
                continue
            pt = rig[HEAD + j * part_width(K):HEAD + (j + 1) * part_width(K)]
            cc = src[idx, 3:6].astype(np.float64) - pt[0:3]
            g0 = ((cc - lo0) * nf0 + 0.5) - tail0
            p0 = ((cc - pt[3:6]) * pt[6:9] + 0.5) - pt[9:12]
            m = idx.size
            heat, u, ori, jc = np.zeros(m), np.zeros((m, 3)), np.zeros((m, 3)), np.full(m, default)
            for k in range(min(max(int(pt[14]), 0), K)):
                e = pt[15 + ENTRY * k:15 + ENTRY * (k + 1)]
                const, origin = e[7] == 1, e[7] == 2
                if const:
                    off = np.full((m, 3), 0.5 * thres)
                else:
                    d = (np.zeros_like(g0) if origin else g0) - e[0:3]
                    dot = (d[:, 0] * e[3] + d[:, 1] * e[4]) + d[:, 2] * e[5]
                    off = dot[:, None] * e[3:6] / e[8] - d
                h = np.sqrt((off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2])
                sel = h > 0 if const else (h <= thres if le else h < thres)
                if origin:                                  # the part's first row only
                    sel = sel & leads[idx]
                hs.append((idx, k, int(e[7]), h))
                heat[sel] = 1.0 - h[sel] / thres
                u[sel] = off[sel] / (h[sel] + 1e-7)[:, None]
                ori[sel] = e[3:6]
                jc[sel] = e[6]
            if rot:
                turn = lambda v, c: (R[:, 0] * (v[:, 0:1] - c) + R[:, 1] * (v[:, 1:2] - c)) + R[:, 2] * (v[:, 2:3] - c) + c
                p0, g0, u, ori = turn(p0, 0.5), turn(g0, 0.5), turn(u, 0.0), turn(ori, 0.0)
            out[idx, 3] = pt[12]
            out[idx, 4:7], out[idx, 7:10], out[idx, 10], out[idx, 11:14], out[idx, 14:17] = p0, g0, heat, u, ori
            out[idx, 17] = pt[13] if pt[13] >= 0 else jc
    return (out, hs) if return_h else out


def frame_of(c):
    """A golden case (gen_point_gt_build_golden.py's dict, or load_case's) as the reference reads it: (f, joints) -- f['gt_points'] /
    f['gt_coords'] dicts of per-link arrays keyed '0', '1', ..., joints the URDF dict of lists (sapien: one xyz list per link)."""
    ends = np.cumsum(c["link_sizes"])
    cut = lambda a: {str(i): np.asarray(a[e - s:e]) for i, (s, e) in enumerate(zip(c["link_sizes"], ends))}
    f = {"gt_points": cut(c["points"]), "gt_coords": cut(c["coords"])}
    xyz = [[float(v) for v in x] for x in c["link_xyz"]]
    n = len(c["axis"])
    joints = {"link": {"xyz": [[x] for x in xyz] if c["dataset"] == "sapien" else xyz},
              "joint": {"axis": [[float(v) for v in a] for a in c["axis"]], "parent": [int(p) for p in c["parent"]],
                        "type": [str(t) for t in c["type"]], "rpy": [[float(v) for v in r] for r in c["rpy"]],
                        "xyz": [[0.0, 0.0, 0.0]] * n, "child": list(range(n))}}
    return f, joints


def store_case(out, c):
    """The inputs of a case as plain arrays under '<name>_<field>' (no pickles)."""
    p = c["name"] + "_"
    out[p + "dataset"] = np.asarray(c["dataset"])
    out[p + "parts_map"] = np.asarray([i for g in c["parts_map"] for i in g], np.int32)
    out[p + "group_sizes"] = np.asarray([len(g) for g in c["parts_map"]], np.int32)
    out[p + "link_sizes"] = np.asarray(c["link_sizes"], np.int32)
    out[p + "points"], out[p + "coords"] = np.asarray(c["points"], np.float32), np.asarray(c["coords"], np.float32)
    out[p + "corners"], out[p + "factors"] = np.asarray(c["corners"], np.float64), np.asarray(c["factors"], np.float64)
    out[p + "link_xyz"], out[p + "axis"] = np.asarray(c["link_xyz"], np.float64), np.asarray(c["axis"], np.float64)
    out[p + "parent"], out[p + "type"], out[p + "rpy"] = np.asarray(c["parent"], np.int32), np.asarray(c["type"]), np.asarray(c["rpy"], np.float64)
    out[p + "target_order"] = np.asarray([] if c["target_order"] is None else c["target_order"], np.int32)


def load_case(z, name):
    """-> the case dict of store_case (and every other '<name>_*' array under its field name)."""
    p = name + "_"
    c = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    c["name"], c["dataset"] = name, str(c["dataset"])
    ends = np.cumsum(c["group_sizes"])
    c["parts_map"] = [[int(i) for i in c["parts_map"][e - s:e]] for s, e in zip(c["group_sizes"], ends)]
    c["link_sizes"] = [int(s) for s in c["link_sizes"]]
    c["target_order"] = [int(i) for i in c["target_order"]] or None
    return c


def build_batch(clouds7, rigs, K):
    """-> the concatenated (n_total, 18) float32 rows of a batch."""
    return np.concatenate([build_rows(c, r, K) for c, r in zip(clouds7, rigs)], axis=0)
