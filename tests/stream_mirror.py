"""numpy mirror of the streaming sampler's keyed bijection (include/ancsh_hip.h, ancsh_input_sample_stream)."""
import numpy as np

M64 = (1 << 64) - 1
SAMPLE_TAG = 0xF000000000000000


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _splitmix64_np(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def tiled_size(n_raw, num_points):
    return n_raw if n_raw >= num_points else (num_points // n_raw + 1) * n_raw


def permutation(seed, cloud, T, count=None):
    """pi(0..count-1) (default: all of [0, T)) of cloud `cloud` under key `seed`, int64."""
    s = int(seed) & M64
    keys = [np.uint64(splitmix64(s ^ splitmix64(SAMPLE_TAG | (cloud << 8) | r))) for r in range(4)]
    w = 0
    while (1 << w) < T:
        w += 2
    h = np.uint64(w // 2)
    mask = np.uint64((1 << (w // 2)) - 1)
    x = np.arange(T if count is None else count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        todo = np.ones(x.shape, bool)
        while todo.any():
            y = x[todo]
            L, R = y >> h, y & mask
            for k in keys:
                L, R = R, L ^ (_splitmix64_np(k ^ R) & mask)
            y = (L << h) | R
            x[todo] = y
            todo[todo] = y >= np.uint64(T)
    return x.astype(np.int64)


def sample_perm(seed, cloud, n_raw, num_points):
    """perm_out row of cloud `cloud`: the first num_points values of its bijection of the tiled cloud."""
    return permutation(seed, cloud, tiled_size(n_raw, num_points), num_points)
