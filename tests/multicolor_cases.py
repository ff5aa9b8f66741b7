"""Matrices and a Python model of the multicolour ordering (kry_color_plan),
shared by tests/test_color_plan.py (host), tests/test_gpu_precond_multicolor.py
(device) and tests/golden/make_precond_multicolor.py (the reference runs).
Plain NumPy / SciPy: nothing here loads the library.
"""
import numpy as np
import scipy.sparse

from tests import precond_factored_cases as PC

# name: the colour sizes greedy first-fit in row order gives (computed with
# color_py below)
COLOR_SIZES = {
    "poisson12": [72, 72],
    "poisson40": [800, 800],
    "poisson64": [2048, 2048],
    "stencil12": [864, 864],
    "arrow300": [150, 149, 1],
    "random3000": [610, 571, 533, 468, 370, 270, 137, 37, 4],
    "random20000": [5128, 4758, 4096, 3257, 1997, 698, 66],
}


def matrix(problems, name):
    """A canonical CSR matrix of COLOR_SIZES, from krylov_amd.problems."""
    if name.startswith("poisson"):
        A = problems.poisson2d(int(name[7:]))
    elif name == "stencil12":
        A = problems.stencil15_3d(12)
    elif name == "arrow300":
        A = PC.arrow(300)
    elif name == "random3000":
        A = problems.random_nonsym(3000, 6, 2.0, 0)
    elif name == "random20000":
        A = problems.random_nonsym(20000, 4)
    else:
        raise KeyError(name)
    return PC.canonical(A)


def color_py(A):
    """(colors, perm): colors[i] = the smallest integer >= 0 that is not the
    colour of a neighbour j < i in the stored pattern of A + A^T without the
    diagonal (explicit zeros are edges); perm = the rows by (colour, row)."""
    S = scipy.sparse.csr_matrix(A)
    n = S.shape[0]
    P = scipy.sparse.csr_matrix((np.ones(S.nnz, dtype=np.int8), S.indices, S.indptr), shape=S.shape)
    G = (P + P.T).tocsr()  # values >= 1 on every stored position of either
    ip, ix = G.indptr, G.indices
    colors = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        nb = ix[ip[i]:ip[i + 1]]
        used = set(colors[nb[nb < i]].tolist())
        c = 0
        while c in used:
            c += 1
        colors[i] = c
    perm = np.argsort(colors, kind="stable").astype(np.int32)
    return colors, perm


def rank_of(perm):
    rank = np.empty(perm.shape[0], dtype=np.int32)
    rank[perm] = np.arange(perm.shape[0], dtype=np.int32)
    return rank


def permuted(A, perm):
    """B = A[perm][:, perm], canonical."""
    return PC.canonical(scipy.sparse.csr_matrix(A)[perm][:, perm])


def split_by_rank(A, rank, lower):
    """The entries (i, j) of A with rank[j] <= rank[i] (lower) or >= (upper),
    in A's numbering: a triangle in the elimination order."""
    S = scipy.sparse.coo_matrix(A)
    keep = rank[S.col] <= rank[S.row] if lower else rank[S.col] >= rank[S.row]
    return PC.canonical(scipy.sparse.coo_matrix((S.data[keep], (S.row[keep], S.col[keep])), shape=S.shape).tocsr())


def host_precond_mc(A, spec, dtype, dense=False):
    """The multicolour preconditioner as a reference user writes it: the
    permutation around HostPrecond on B = A[perm][:, perm]."""
    _, perm = color_py(A)
    inner = PC.host_precond(permuted(A, perm), spec, dtype, dense)
    rank = rank_of(perm)

    class Permuted:
        shape = inner.shape
        dtype = inner.dtype

        def __matmul__(self, x):
            return (inner @ np.asarray(x)[perm])[rank]

    return Permuted()
