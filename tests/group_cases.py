"""The case of the first-layer group tests (set_tuning("nll_group")), shared by
the CPU and GPU tests: 7 images in chunks of 2 under groups of 4 images run
the groups [0, 4) and [4, 7) -- the third chunk starts a group in the middle
of the call, the last chunk holds one image.

For iwae_score / iwae_score_grad and their masked forms the case is G7 (S2's
model of score_ref, k = 5) and OG7 (G7 under missing_ref's mask: image 0
entirely missing, image 1 entirely observed), registered in the second
registries of score_ref and observed_ref.  iwae_nll, iwae_posterior and
iwae_impute take N, K, CHUNK, GROUP with the cases of their own files.

A test of the group boundary starts from a model that has run nothing: a
workspace that an earlier call on the same images filled would still hold the
right rows of x and of the first encoder layer where a broken walk reads them."""
import observed_ref as OB
import score_ref as R

N, K, CHUNK, GROUP = 7, 5, 2, 4
GROUP_CASE = "G7"
R.EXTRA_CASES[GROUP_CASE] = (tuple(R.CASES["S2"][0]), N, K, 9707, R.X_DIM, 0.0)
OB.EXTRA_CASES["O" + GROUP_CASE] = (GROUP_CASE,) + tuple(R.EXTRA_CASES[GROUP_CASE][:5]) + (False,)


def counter_deltas(m, ids, call):
    """(call's result, the deltas of the library's launch counters `ids` over it)"""
    c0 = [int(m._lib.iwae_debug_count(m._h, i)) for i in ids]
    out = call()
    return out, [int(m._lib.iwae_debug_count(m._h, i)) - c for i, c in zip(ids, c0)]


def groups_then_one_group(m, ids, call):
    """On a model that has run nothing: call() under groups of GROUP images, then under the default group size
    (one group).  (the first result, the second, the counter deltas of the first call)"""
    m.set_tuning("nll_group", GROUP)
    out, d = counter_deltas(m, ids, call)
    m.set_tuning("nll_group", 16384)
    return out, call(), d
