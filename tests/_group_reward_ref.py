"""Reference of the group reward of self-critical RL on n samples per image (include/insenticap_hip.h, isc_group_reward;
rewards.get_group_self_critical_reward): the formulas restated in numpy float64 with explicit loops in the stated order.

  baseline[i,j] = (sum over k != j, k ascending, of scores[i,k]) / (n - 1)
  adv[i,j]      = scores[i,j] - baseline[i,j]
  reward[r,t]   = (float32)(adv[r] + cls_flag * (float64)cls_reward[r,t])        ((float32)adv[r] without a classifier term)
  stats4        = mean scores, mean adv, mean cls_reward over all I*n*T entries (0 without one), mean of the float32 reward
                  values - every sum accumulated in float64, rows ascending, steps ascending inside.
"""
import numpy as np


def advantages(scores, n):
    """float64 [I*n] -> float64 [I*n], one scalar operation at a time."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1, n)
    adv = np.empty_like(s)
    for i in range(s.shape[0]):
        for j in range(n):
            acc = np.float64(0.0)
            for k in range(n):
                if k != j:
                    acc = acc + s[i, k]
            adv[i, j] = s[i, j] - acc / np.float64(n - 1)
    return adv.reshape(-1)


def group_reward(scores, n, T, cls_reward=None, cls_flag=0.0):
    """Returns (adv float64 [I*n], reward float32 [I*n, T], stats4 float64 [4])."""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    rows = scores.shape[0]
    adv = advantages(scores, n)
    reward = np.empty((rows, T), dtype=np.float32)
    for r in range(rows):
        for t in range(T):
            if cls_reward is None:
                reward[r, t] = np.float32(adv[r])
            else:
                term = np.float64(cls_flag) * np.float64(cls_reward[r, t])
                reward[r, t] = np.float32(adv[r] + term)
    sums = [np.float64(0.0)] * 4
    for r in range(rows):
        sums[0] = sums[0] + scores[r]
        sums[1] = sums[1] + adv[r]
        for t in range(T):
            if cls_reward is not None:
                sums[2] = sums[2] + np.float64(cls_reward[r, t])
            sums[3] = sums[3] + np.float64(reward[r, t])
    stats4 = np.array([sums[0] / rows, sums[1] / rows, sums[2] / (rows * T), sums[3] / (rows * T)], dtype=np.float64)
    return adv, reward, stats4


def stats_bounds(scores, adv, reward, cls_reward):
    """The issue's bound per stats4 entry: N * 2^-53 * sum|x| over the N terms of that entry's sum - the error bound of an
    N-term float64 sum in any order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: (N - 1) u sum|x|)."""
    u = 2.0 ** -53
    out = []
    for x in (scores, adv, cls_reward, reward):
        if x is None:
            out.append(0.0)
        else:
            a = np.abs(np.asarray(x, dtype=np.float64)).reshape(-1)
            out.append(a.size * u * float(a.sum()))
    return out


def make_scores(I, n, seed):
    """Scores with ties inside an image, zeros and values up to 10."""
    rng = np.random.default_rng(seed)
    s = rng.random((I, n)) * 10.0
    s[0, :] = s[0, 0]                         # image 0: all samples tie
    if I > 1:
        s[1, :] = 0.0                         # image 1: all zeros
        s[1, -1] = 10.0                       # ... but one at the top of the range
    if I > 2:
        s[2, 0] = 0.0
        if n > 2:
            s[2, 1] = s[2, 2]                 # a tie of two inside an image
    return s.reshape(-1)
