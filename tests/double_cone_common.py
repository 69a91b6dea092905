"""Shared by the DoubleCone tests and tests/golden/make_golden_double_cone.py.

The small DoubleCone networks of the fixtures have ~300,000 parameters, so full copies of their
weights and gradients would not fit the repository's file-size limit.  A tensor of at most SMALL
elements is recorded in full; a larger one as SAMPLE evenly spaced elements of its flattened values
plus its moments (sum, sum of squares, max |.|, in float64).  The tests compare the recorded elements
one by one and the moments within what the element-wise tolerance implies for them."""
import numpy as np

NVEC = np.array([6, 4, 4, 4, 4, 7, 49])
SUB = {0: {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 5}}
SMALL_KW = dict(backbone_channels=32, pooled_channels=64, in_num_res_blocks=1, cone_num_res_blocks=2,
                out_num_res_blocks=1, critic_channels=16, additional_critic_activation_functions=["tanh", "identity"],
                subaction_mask=SUB)
SMALL, SAMPLE = 1024, 512
FLAT_SAMPLE = 8192  # elements recorded of a flat parameter vector (the PPO steps fixture)


def sample_idx(n: int, small: int = SMALL, sample: int = SAMPLE) -> np.ndarray:
    if n <= small:
        return np.arange(n)
    return np.linspace(0, n - 1, sample).astype(np.int64)


def sampled(a) -> np.ndarray:
    a = np.asarray(a).reshape(-1)
    return a[sample_idx(a.size)].copy()


def moments(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    return np.array([a.sum(), (a * a).sum(), np.abs(a).max() if a.size else 0.0])


def check_moments(got, ref_m, el_tol: float, name: str = "") -> None:
    """`got` against recorded moments, given a per-element tolerance el_tol: the sum within n * el_tol,
    the norm within sqrt(n) * el_tol."""
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    n = g.size
    assert abs(g.sum() - ref_m[0]) <= n * el_tol, (name, g.sum(), ref_m[0])
    assert abs(np.sqrt((g * g).sum()) - np.sqrt(ref_m[1])) <= np.sqrt(n) * el_tol, (name, (g * g).sum(), ref_m[1])
