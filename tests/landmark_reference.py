"""NumPy / scipy restatement of the landmark algebra (graphtools 1.5.x ``LandmarkGraph.build_landmark_op`` / ``extend_to_data``,
restated from its definition; nothing is copied): the host reference of tests/test_landmark_host.py and tests/test_gpu_landmark.py.

With ``K`` the symmetric kernel with its diagonal, ``c`` the labels in ``[0, L)`` and ``C`` their one-hot ``[N, L]``:
``A = K C``, ``transitions = diag(1 / r) A`` with ``r = A 1``, ``pmn = diag(1 / s) A^T`` with ``s = A^T 1``,
``landmark_op = pmn @ transitions``."""
import numpy as np
from scipy import sparse


def onehot(labels, L):
    labels = np.asarray(labels)
    n = labels.shape[0]
    return sparse.csr_matrix((np.ones(n), (np.arange(n), labels)), shape=(n, int(L)))


def merged(K, labels, L):
    """``K C`` as CSR with sorted indices (``K`` may be rectangular ``[M, N]``: the kernel rows of new cells)."""
    A = sparse.csr_matrix(sparse.csr_matrix(K) @ onehot(labels, L))
    A.sum_duplicates()
    A.sort_indices()
    return A


def l1_rows(A):
    """Rows divided by their sums; a row that sums to zero stays as it is (sklearn's ``normalize(A, "l1")`` on non-negative rows)."""
    A = sparse.csr_matrix(A)
    r = np.asarray(A.sum(1)).ravel()
    return (sparse.diags(1.0 / np.where(r > 0, r, 1.0)) @ A).tocsr()


def landmark_algebra(K, labels, L):
    """dict(A, r, s, transitions, pmn, landmark_op): ``landmark_op`` dense ``[L, L]``, the others sparse / vectors."""
    A = merged(K, labels, L)
    r = np.asarray(A.sum(1)).ravel()
    s = np.asarray(A.sum(0)).ravel()
    pnm = l1_rows(A)
    pmn = l1_rows(A.T.tocsr())
    op = np.asarray((pmn @ pnm).todense())
    return dict(A=A, r=r, s=s, transitions=pnm, pmn=pmn, landmark_op=op)


def brute_force(K, labels, L):
    """graphtools' definition on dense arrays: per-cluster sums of the kernel's rows (``pmn``), its transpose (``pnm``), two l1
    normalisations, one product."""
    Kd = np.asarray(sparse.csr_matrix(K).todense())
    labels = np.asarray(labels)
    pmn = np.zeros((L, Kd.shape[1]))
    for l in range(L):
        pmn[l] = Kd[labels == l].sum(axis=0)
    pnm = pmn.T.copy()
    pmn = pmn / np.where(pmn.sum(1) > 0, pmn.sum(1), 1.0)[:, None]
    pnm = pnm / np.where(pnm.sum(1) > 0, pnm.sum(1), 1.0)[:, None]
    return dict(transitions=pnm, pmn=pmn, landmark_op=pmn @ pnm)
