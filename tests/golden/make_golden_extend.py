#!/usr/bin/env python
"""Regenerate tests/golden/g9_extend.npz: kernels from NEW cells to fitted cells, from the CPU oracle.

    python tests/golden/make_golden_extend.py

``oracle.kernel_to_data`` restates [UPSTREAM graphtools 1.5.x ``kNNGraph.build_kernel_to_data``] for queries that are not
among the references; the fixture holds 600 x 8 fitted cells, three query sets (150 cells with 3 exact copies of fitted cells and
5 far outliers, 63 cells, 1 cell), the kernels of three parameter sets as CSR triplets, their row-normalised products with a
fixed random F for p in {1, 3, 7}, a 600 x 40 -> n_pca = 8 case with the oracle's exact PCA, and one fit_transform (densities on
the fitted cells, interpolated to the 150 new ones).

The oracle runs with its default tree search, whose distances are direct differences: sklearn's brute route forms them from the
norms and loses 1e-8 (relative, in the kernel value) on the clumps of fitted cells that lie 200 units from the rest.

Size: the file stays within three quarters of g6_c2mini_5000x50.npz (``size_bound``; the generator refuses to write a larger one
and tests/test_extend_host.py checks the committed file).  The kernels' values are fp64 as the oracle gave them; the inputs are
multiples of 2^-10 (float32, exactly), F multiples of 1/8 (float16, exactly); the products and the densities, which the tests
compare at 1e-5, are kept as float32.

The generator refuses to write a fixture whose sparsity pattern is not well defined: no stored value within a relative 1e-6
above thresh, no excluded pair within a relative 1e-9 of the radius -- so a test may demand the identical pattern.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import meld_oracle as mo  # noqa: E402

N_REF, D = 600, 8
PARAMS = {"a": dict(knn=5, decay=40, thresh=1e-4), "b": dict(knn=5, decay=None, thresh=1e-4), "w": dict(knn=20, decay=2, thresh=1e-4)}
QUERIES = ("q150", "q63", "q1")
P_LIST = (1, 3, 7)
COPIES = (7, 311, 599)  # fitted cells repeated among the 150 new ones (rows 10, 11, 12 of q150)
N_OUT = 5  # far outliers: the last rows of q150
N_CLUMPS, CLUMP = 6, 22  # remote clumps of fitted cells: the last N_CLUMPS * CLUMP of them
# "well under the size of g6_c2mini_5000x50.npz": three quarters of it at the most.  (What the fixture has to hold does not go
# far below that: (20 + 5) kernel values x 214 new cells in fp64 are 43 kB before a single row is longer than its knn.)
SIZE_OF = "g6_c2mini_5000x50.npz"
SIZE_NUM, SIZE_DEN = 3, 4


def size_bound():
    return os.path.getsize(os.path.join(HERE, SIZE_OF)) * SIZE_NUM // SIZE_DEN


def f32(a):
    """Rounded to multiples of 2^-10, which float32 holds exactly (the fixture stores its inputs as float32, and the zero bits
    at the end of each compress)."""
    r = np.round(np.asarray(a, dtype=np.float64) * 1024.0) / 1024.0
    assert np.array_equal(r.astype(np.float32).astype(np.float64), r)
    return r


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pca_cells():
    """The raw 600 + 63 cells x 40 of the PCA case: regenerated from the seeded generator (their checksum is stored)."""
    Xp, _ = mo.synthetic_cells(N_REF + 63, n_dims=40, seed=11)
    return f32(Xp)


def make_cells():
    """Fitted cells, labels and the three query sets.

    The kernel values are fp64 and do not compress, and a wide row (knn = 20, decay = 2: a radius of 3 bandwidths) holds 60
    entries and more wherever the data goes on, so the fixture's size is the number of wide entries.  The cells therefore lie
    along one latent coordinate (``latent_dim=1``) in 8 dimensions, and the last N_CLUMPS x CLUMP fitted cells form small remote
    clumps, 200 units out along one axis each: a new cell in a clump reaches its CLUMP cells and nothing else, the shortest wide
    row there is (knn = 20 needs 20 of them).  Most new cells are drawn in the clumps; a few come from the pool along the
    latent coordinate, two of them with rows beyond 80 entries.  A far outlier would see ALL the data at about the same relative
    distance, so the outliers are far (100 clump spacings) from the last clump, which is all their radius reaches."""
    X, labels = mo.synthetic_cells(N_REF + 600, n_dims=D, seed=9, latent_dim=1)
    X = f32(X)
    ref, lab = X[:N_REF].copy(), labels[:N_REF].copy()
    rng = np.random.default_rng(7)
    centres = ref.mean(0) + 200.0 * np.eye(D)[:N_CLUMPS]
    for k in range(N_CLUMPS):
        ref[N_REF - (N_CLUMPS - k) * CLUMP:N_REF - (N_CLUMPS - k - 1) * CLUMP] = f32(centres[k] + 0.05 * rng.normal(size=(CLUMP, D)))
    pool = X[N_REF:]
    wide = np.diff(mo.kernel_to_data(pool, ref, **PARAMS["w"]).indptr)
    long_rows = np.nonzero((wide > 80) & (wide <= 120))[0][:2]
    short_rows = np.sort(np.setdiff1d(np.argsort(wide, kind="stable")[:20], long_rows)[:14])
    assert len(long_rows) == 2 and len(short_rows) == 14

    def in_clumps(n):
        return f32(centres[rng.integers(0, N_CLUMPS, size=n)] + 0.05 * rng.normal(size=(n, D)))

    q150 = np.concatenate([pool[long_rows], pool[short_rows[:8]], in_clumps(150 - 10)])
    q150[10:13] = ref[list(COPIES)]
    dirs = rng.normal(size=(N_OUT, D))
    q150[-N_OUT:] = f32(centres[-1] + 5.0 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True))
    q63 = np.concatenate([pool[short_rows[8:13]], in_clumps(63 - 5)])
    q1 = pool[short_rows[13:14]].copy()
    return ref, lab, dict(q150=q150, q63=q63, q1=q1)


def pairwise(Q, R):
    return np.sqrt(((Q[:, None, :] - R[None, :, :]) ** 2).sum(-1))


def check_pattern(K, Q, R, knn, decay, thresh):
    """The assertions that make the pattern well defined (shared with tests/test_extend_host.py through the stored arrays)."""
    assert K.shape == (Q.shape[0], R.shape[0])
    lens = np.diff(K.indptr)
    assert lens.max() <= 128, "a row exceeds the 128-entry candidate list: {}".format(lens.max())
    if decay is None:
        assert (lens == knn).all()
        dist = np.sort(pairwise(Q, R), axis=1)
        gap = (dist[:, knn] - dist[:, knn - 1]) / dist[:, knn]
        assert gap.min() > 1e-9, "a tie at the knn-th neighbour"
        return
    assert not ((K.data >= thresh) & (K.data <= thresh * (1 + 1e-6))).any(), "a stored value sits on the threshold"
    dist = pairwise(Q, R)
    bw = np.maximum(np.sort(dist, axis=1)[:, knn - 1], np.finfo(float).eps)
    radius = bw * (-np.log(thresh)) ** (1.0 / decay)
    stored = np.asarray(K.todense()) > 0
    rel = np.abs(dist - radius[:, None]) / radius[:, None]
    assert rel[~stored].min() > 1e-9, "an excluded pair lies on the radius"
    assert (dist[stored] <= radius[:, None].repeat(R.shape[0], 1)[stored]).all()


def main():
    ref, labels, queries = make_cells()
    out = dict(ref=ref, labels=labels, copies=np.array(COPIES), copy_rows=np.array([10, 11, 12]), n_outliers=np.array(N_OUT))
    rng = np.random.default_rng(2024)
    F = rng.integers(-16, 17, size=(N_REF, max(P_LIST))) / 8.0  # (random multiples of 1/8: float16 holds them exactly)
    out["F"] = F
    for q, Q in queries.items():
        out[q] = Q
        for tag, par in PARAMS.items():
            K = mo.kernel_to_data(Q, ref, **par).tocsr()
            K.sort_indices()
            check_pattern(K, Q, ref, **par)
            out["K_{}_{}_indptr".format(tag, q)] = K.indptr.astype(np.int64)
            out["K_{}_{}_indices".format(tag, q)] = K.indices.astype(np.int16)
            out["K_{}_{}_data".format(tag, q)] = K.data.astype(np.float64)
            T = K.multiply(1.0 / np.asarray(K.sum(1))).tocsr()
            # (its first p columns are the product with F[:, :p], p in P_LIST; float32, 6e-8 of a tolerance of 1e-5)
            out["TF_{}_{}".format(tag, q)] = np.asarray(T @ F).astype(np.float32)
    wide = np.diff(out["K_w_q150_indptr"])
    assert wide.max() > 64, "the wide case has no row beyond 64 entries: {}".format(wide.max())
    for r, c in zip((10, 11, 12), COPIES):  # a copy of a fitted cell gets 1 there
        row = slice(out["K_a_q150_indptr"][r], out["K_a_q150_indptr"][r + 1])
        assert out["K_a_q150_data"][row][list(out["K_a_q150_indices"][row]).index(c)] == 1.0

    # PCA case: 600 x 40 raw cells, the oracle's exact PCA to 8 components (sklearn svd_solver="full"), new cells raw and reduced
    from sklearn.decomposition import PCA

    Xp = pca_cells()
    raw_ref, raw_q = Xp[:N_REF], Xp[N_REF:]
    pca = PCA(8, svd_solver="full").fit(raw_ref)
    red_ref, red_q = pca.transform(raw_ref), pca.transform(raw_q)
    Kp = mo.kernel_to_data(red_q, red_ref, **PARAMS["a"]).tocsr()
    Kp.sort_indices()
    check_pattern(Kp, red_q, red_ref, **PARAMS["a"])
    out.update(pca_raw_sha=np.array(sha(Xp)), pca_red_q=red_q, K_pca_indptr=Kp.indptr.astype(np.int64),
               K_pca_indices=Kp.indices.astype(np.int16), K_pca_data=Kp.data.astype(np.float64))

    # one fit_transform on the fitted cells and its densities interpolated to the 150 new cells
    samples, dens, G = mo.fit_transform(ref, labels, return_graph=True, **PARAMS["a"])
    Ka = mo.kernel_to_data(queries["q150"], ref, **PARAMS["a"]).tocsr()
    Ta = Ka.multiply(1.0 / np.asarray(Ka.sum(1))).tocsr()
    out.update(samples=np.asarray(samples), lmax=np.array(G.lmax), dens=np.asarray(dens).astype(np.float32),
               dens_q150=np.asarray(Ta @ dens).astype(np.float32))  # (compared at 1e-5: float32 is 6e-8)

    for k in ("ref", "F") + QUERIES:  # (float32 holds them exactly: f32(); F even in float16)
        t = np.float16 if k == "F" else np.float32
        assert np.array_equal(out[k].astype(t).astype(np.float64), out[k]), k
        out[k] = out[k].astype(t)
    path = os.path.join(HERE, "g9_extend.npz")
    np.savez_compressed(path + ".tmp.npz", **out)
    size = os.path.getsize(path + ".tmp.npz")
    if size > size_bound():
        os.remove(path + ".tmp.npz")
        raise AssertionError("the fixture would be {} bytes, beyond {}/{} of {} ({})".format(size, SIZE_NUM, SIZE_DEN, SIZE_OF, size_bound()))
    os.replace(path + ".tmp.npz", path)
    print("wrote {} ({} bytes); wide rows: max {} entries, {} rows beyond 64".format(path, os.path.getsize(path), wide.max(), int((wide > 64).sum())))


if __name__ == "__main__":
    main()
