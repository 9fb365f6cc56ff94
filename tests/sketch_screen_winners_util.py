"""Host-side oracle of the winner-takes-all screen (kmc_sketch_screen_winners): the rule of
include/kmc.h restated with numpy on top of sketch_screen_util.multiplicities.  The ranking
is computed in Python integers (all[a] * size[b] against all[b] * size[a], then the smaller
index); the identity as sketch_screen_util computes it.  After it, the helpers the test
files share.  No device code."""
import numpy as np

import sketch_screen_util as U


def winners_expected(mix, rows, sizes, s, k):
    """(won uint32 [n], median_won uint32 [n], identity_won float32 [n], all uint32 [n])."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, s)
    n = rows.shape[0]
    size = [min(int(sizes[r]), s) for r in range(n)]
    mult = [U.multiplicities(mix, rows[r, :size[r]]) for r in range(n)]
    all_ = [int((m > 0).sum()) for m in mult]
    winner = {}  # found value -> the first row of the ranking that holds it
    for r in range(n):
        if all_[r] == 0:
            continue
        for v in rows[r, :size[r]][mult[r] > 0]:
            v = int(v)
            w = winner.get(v)
            if w is None:
                winner[v] = r
                continue
            a, b = all_[r] * size[w], all_[w] * size[r]
            if a > b or (a == b and r < w):
                winner[v] = r
    won = np.zeros(n, dtype=np.uint32)
    median = np.zeros(n, dtype=np.uint32)
    ident = np.zeros(n, dtype=np.float32)
    for r in range(n):
        mine = np.array([winner.get(int(v)) == r for v in rows[r, :size[r]]], dtype=bool) & (mult[r] > 0)
        m = np.sort(mult[r][mine])
        won[r] = m.size
        if m.size:
            median[r] = m[(m.size - 1) // 2] & 0xFFFFFFFF
        ident[r] = U.identity_formula(m.size, size[r], k)
    return won, median, ident, np.array(all_, dtype=np.uint32)


def contested(mix, rows, sizes, s):
    """The found values that more than one row holds within its size."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, s)
    held = np.concatenate([rows[r, :min(int(sizes[r]), s)] for r in range(rows.shape[0])] + [np.zeros(0, np.uint64)])
    values, times = np.unique(held, return_counts=True)
    values = values[times > 1]
    return values[U.multiplicities(mix, values) > 0]


def host_winners(res):
    """kmc.sketch_screen_winners' tensors on the host: (won, median, identity, all), None kept."""
    won, med, ident, sh = res
    u32 = lambda t: t.cpu().numpy().view(np.uint32) if t is not None else None
    return u32(won), u32(med), ident.cpu().numpy() if ident is not None else None, u32(sh)


def assert_winners(got, exp, msg=""):
    """Integers bit for bit, the identity by sketch_screen_util.assert_identity; an output
    that was not asked for (None) is not compared."""
    np.testing.assert_array_equal(got[0], exp[0], err_msg="%s won" % msg)
    if got[1] is not None:
        np.testing.assert_array_equal(got[1], exp[1], err_msg="%s median_won" % msg)
    if got[2] is not None:
        U.assert_identity(got[2], exp[2], "%s identity_won" % msg)
    if got[3] is not None:
        np.testing.assert_array_equal(got[3], exp[3], err_msg="%s all" % msg)
