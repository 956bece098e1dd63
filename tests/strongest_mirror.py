"""NumPy restatement of strongest-N for SIFT and SURF (DESIGN.md "Strongest-N for SIFT and SURF") -- test infrastructure, not a
test.  The candidates are the rows of the unselected result (oracle.sift, tests/surf_mirror.py) in canonical order, the strength
is aux[:, 2] as f32, and the rule keeps the first min(N, count) candidates by (strength descending, canonical index ascending),
in canonical order."""
import numpy as np


def keep(resp, N):
    """Indices of the kept rows, ascending.  The stable sort of the negated strengths breaks ties towards the lower index."""
    if N < 1:
        raise ValueError("NumStrongest must be at least 1")
    resp = np.asarray(resp)
    assert resp.dtype == np.float32 and resp.ndim == 1 and not (resp < 0).any()
    return np.sort(np.argsort(-resp.astype(np.float64), kind='stable')[:N])


def pick(result, N):
    """(desc, loc, aux) of the unselected result -> (desc, loc, aux) of the call with NumStrongest = N."""
    d, loc, aux = result
    k = keep(aux[:, 2], N)
    return d[k], loc[k], aux[k]


def tie_cuts(aux, loc, cross=True):
    """The cuts N (1 <= N < count) that fall inside a tie: the N-th and the (N + 1)-th row in strength order have the same
    strength.  cross=True: only ties between rows of different keypoints (location, size or layer differ); cross=False: only
    ties between the orientations of one keypoint (SIFT)."""
    resp = aux[:, 2]
    order = np.argsort(-resp.astype(np.float64), kind='stable')
    same_kp = lambda a, b: bool(np.array_equal(loc[a], loc[b]) and aux[a, 0] == aux[b, 0] and aux[a, 3] == aux[b, 3])  # noqa: E731
    return [n for n in range(1, len(order)) if resp[order[n - 1]] == resp[order[n]] and same_kp(order[n - 1], order[n]) != cross]
