"""Integer oracle of rai_ref_actions_store (csrc/ref_actions.hip) and the case list its tests share
(test_gpu_ref_actions_kernel.py: the kernel; test_reference_rollout_cpu.py: the host twin).  No floats: the
oracle walks the components one by one in Python integers."""
import numpy as np

GRID_NVEC = (6, 4, 4, 4, 4, 7, 49)
INT32_MAX = 2**31 - 1


def oracle(src, nvec, mask, cells):
    """(dst int64 (R, G), bad int32 (N,)): out of range -> 0, counted; in range, the group's slice has a true
    entry and the action's entry is false -> kept, counted; otherwise kept."""
    nvec = [int(n) for n in nvec]
    G, A = len(nvec), sum(nvec)
    a = np.asarray(src).reshape(-1, G)
    R = a.shape[0]
    assert R % cells == 0
    m = None if mask is None else np.asarray(mask).reshape(R, A)
    dst = np.zeros((R, G), dtype=np.int64)
    bad = np.zeros(R // cells, dtype=np.int32)
    off = [0]
    for n in nvec:
        off.append(off[-1] + n)
    for r in range(R):
        for g in range(G):
            v = int(a[r, g])
            if v < 0 or v >= nvec[g]:
                bad[r // cells] += 1
                continue
            dst[r, g] = v
            if m is not None:
                sl = m[r, off[g]:off[g + 1]]
                if bool(sl.any()) and not bool(sl[v]):
                    bad[r // cells] += 1
    return dst, bad


# (name, nvec, cells, N): GridNet planes over one cell, a few, more than half a tile of 64 rows and four tiles;
# Discrete and MultiDiscrete rows at one env, more than one tile / workgroup of 256, and one past four workgroups
SHAPES = ([(f"grid_c{c}_n{n}", GRID_NVEC, c, n) for c in (1, 4, 37, 256) for n in (1, 3, 65)]
          + [(f"disc_n{n}", (6,), 1, n) for n in (1, 67, 1025)]
          + [(f"md_n{n}", (3, 5, 2), 1, n) for n in (1, 130)])


def make_case(nvec, cells, N, dtype, with_mask, seed):
    """(src (N * cells, G) of dtype, mask (N * cells, A) bool or None).  Legal bot-like actions first, then the
    injections: negative values, a == nvec[g], INT32_MAX, for int64 sources 2**32 + 1 and -(2**40), in-range
    masked-out values, all-false groups, all-false rows; env 0 has nothing wrong and the last env (when there
    is more than one) has every component wrong."""
    rng = np.random.default_rng(seed)
    nv = np.asarray(nvec, dtype=np.int64)
    G, A, R = len(nv), int(nv.sum()), N * cells
    off = np.concatenate([[0], np.cumsum(nv)])
    mask = None
    if with_mask:
        mask = rng.random((R, A)) < 0.6
        dead_rows = rng.random(R) < 0.2
        mask[dead_rows] = False  # all-false rows
        for g in range(G):  # all-false groups inside live rows
            mask[rng.random(R) < 0.15, off[g]:off[g + 1]] = False
    # legal actions: a valid entry where the group has one, anything in range otherwise
    src = np.zeros((R, G), dtype=np.int64)
    for g in range(G):
        pick = rng.integers(0, nv[g], size=R)
        if mask is not None:
            mg = mask[:, off[g]:off[g + 1]]
            first = mg.argmax(axis=1)
            ok = np.take_along_axis(mg, pick[:, None], axis=1)[:, 0]
            pick = np.where(mg.any(axis=1) & ~ok, first, pick)
        src[:, g] = pick
    # injections, everywhere but env 0
    wrong = [-1, -7, None, INT32_MAX]  # None: a == nvec[g]
    if np.dtype(dtype) == np.int64:
        wrong += [2**32 + 1, -(2**40), 2**32]
    inj = rng.random((R, G)) < 0.25
    inj[:cells] = False
    kind = rng.integers(0, len(wrong) + 2, size=(R, G))  # the last two kinds: masked-out in-range values
    for r, g in zip(*np.nonzero(inj)):
        k = int(kind[r, g])
        if k < len(wrong):
            src[r, g] = int(nv[g]) if wrong[k] is None else wrong[k]
        elif mask is not None:
            mg = mask[r, off[g]:off[g + 1]]
            if mg.any() and not mg.all():
                src[r, g] = int(np.argmin(mg))
    if N > 1:  # the last env: every component wrong (out of range, or masked out where the group allows)
        lo = (N - 1) * cells
        for r in range(lo, R):
            for g in range(G):
                mg = None if mask is None else mask[r, off[g]:off[g + 1]]
                if mg is not None and mg.any() and not mg.all() and (r + g) % 2:
                    src[r, g] = int(np.argmin(mg))
                else:
                    src[r, g] = wrong[(r + g) % len(wrong)] if wrong[(r + g) % len(wrong)] is not None else int(nv[g])
    return src.astype(dtype), mask


def cases():
    """Every shape x both source dtypes x mask / no mask: (id, nvec, cells, N, dtype, with_mask, seed)."""
    out = []
    for i, (name, nvec, cells, N) in enumerate(SHAPES):
        for dtype in (np.int32, np.int64):
            for with_mask in (False, True):
                out.append((f"{name}_{np.dtype(dtype).name}_{'mask' if with_mask else 'nomask'}", nvec, cells, N,
                            dtype, with_mask, 100 + i))
    return out
