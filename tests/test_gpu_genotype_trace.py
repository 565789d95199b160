"""GPU: the matrices of genotype_kernel (otg_genotype_cluster_trace_batch) against a plain numpy restatement of anallele_cluster's
arithmetic (src/otterclust.cpp:322-420, src/anseqs.cpp:111-166), operation for operation and bit for bit: 3-mer counts with the 65th bin,
`total` as an int, frequencies, the norm summed over the 65 bins in order, sqrt, the dot product summed in order,
1 - round(cs * 1000) / 1000 with C's round (libm through ctypes: numpy rounds half to even), the NaN-norm rule, the length ratio.  Division
and sqrt are correctly rounded on both sides.  The merge heights of the two clusterings against ref_hclust_average on those matrices.
The dot product itself is not an output: it shows only through the cosine distance, which is rounded to three decimals.
hsd goes through the device log / pow and keeps its 1e-9 relative tolerance (test_gpu_genotype.py)."""
import ctypes as C
import ctypes.util
import numpy as np
import pytest
from otter_amd import abi
from helpers import mutate, tr_seq
import oracle_lib

pytestmark = pytest.mark.gpu

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.round.restype = C.c_double
_libm.round.argtypes = [C.c_double]
_CODE = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i      # lower case


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _seqsum(m):
    """left-to-right sum over the last axis, starting from 0.0 (np.sum is pairwise)"""
    return np.cumsum(m, axis=-1)[..., -1]


def _expected(seqs):
    """(kvec, vnorm, dl, dk) of one region"""
    A = len(seqs)
    kv = np.zeros((A, 65))
    for a, s in enumerate(seqs):
        c = _CODE[np.frombuffer(s, dtype=np.uint8)]
        if c.size >= 3:
            ok = (c[:-2] != 4) & (c[1:-1] != 4) & (c[2:] != 4)
            idx = np.where(ok, 16 * (c[:-2] & 3) + 4 * (c[1:-1] & 3) + (c[2:] & 3), 64)
            kv[a] = np.bincount(idx, minlength=65)
    total = kv.sum(axis=1).astype(np.int64)                      # int total_counts (small integers: exact in any order)
    with np.errstate(invalid="ignore", divide="ignore"):
        kv = kv / total[:, None].astype(np.float64)
        vn = np.sqrt(_seqsum(kv * kv))
        i, j = np.triu_indices(A, 1)
        ln = np.array([len(s) for s in seqs], dtype=np.int64)
        x, y = ln[i], ln[j]
        dl = np.where(x < y, (y - x).astype(np.float64) / y, (x - y).astype(np.float64) / x)
        cs = _seqsum(kv[i] * kv[j]) / (vn[i] * vn[j])
        nan_norm = np.isnan(vn[i]) | np.isnan(vn[j])
        rounded = np.array([0.0 if q else _libm.round(float(v)) / 1000.0 for v, q in zip((cs * 1000.0).tolist(), nan_norm.tolist())])
        dk = 1.0 - rounded
    return kv, vn, dl, dk


def _region(rng, A, short_at=None, n_at=None):
    pop = [tr_seq(rng, int(rng.integers(80, 400))) for _ in range(4)]
    seqs = []
    for a in range(A):
        s = mutate(rng, pop[int(rng.integers(0, 4))], [0.0, 0.004, 0.03][a % 3]) or b"A"
        if a == short_at:
            s = s[:int(rng.integers(0, 3))]
        if a == n_at:
            s = s[:7] + b"NnN" + s[7:] + b"acgtacg"
        seqs.append(s)
    return seqs


def test_genotype_matrices(gpu, oracle):
    """A = 2, 3 (the smallest matrices), 102 (5 151 pairs: the last size clustered in LDS), 103 (the first in HBM, whose cosine matrix the
    product path clusters in place), 1 (no matrix) and 257 (the wide kernel), with one allele of length 0-2 (NaN norm) and one holding N."""
    rng = np.random.default_rng(81)
    regions = [_region(rng, 2, n_at=1), _region(rng, 3, short_at=1), _region(rng, 102, short_at=40, n_at=3), _region(rng, 103, short_at=0, n_at=102),
               _region(rng, 1), _region(rng, 3, short_at=2, n_at=0), _region(rng, 257, short_at=200, n_at=256)]
    assert {len(s) for r in regions for s in r} & {0, 1, 2}
    seqs = [s for r in regions for s in r]
    counts = np.array([len(r) for r in regions], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
    arena, off, ln = abi.pack_seqs(seqs)
    P = abi.default_params()
    args = (arena, off, ln, first, counts)
    out, tr = gpu.genotype_cluster_trace_batch(P, *args)
    plain = gpu.genotype_cluster_batch(P, *args)
    ora = oracle.genotype_cluster_batch(P, *args)
    for q in (0, 1, 2, 4, 5):
        assert np.array_equal(out[q], plain[q]) and np.array_equal(out[q], ora[q]), q
    assert _same(out[3], plain[3]) and np.allclose(out[3], ora[3], rtol=1e-9, atol=0, equal_nan=True)
    src = "ref" if oracle_lib.ref() is not None else "oracle"
    p0 = 0
    saw_nan = False
    for r, rs in enumerate(regions):
        A, f = len(rs), int(first[r])
        kv, vn, dl, dk = _expected(rs)
        npair = A * (A - 1) // 2
        assert _same(tr["kvec"][f:f + A], kv), (r, A)
        assert _same(tr["vnorm"][f:f + A], vn), (r, A)
        saw_nan |= bool(np.isnan(vn).any())
        assert _same(tr["dl"][p0:p0 + npair], dl), (r, A, np.flatnonzero(_bits(tr["dl"][p0:p0 + npair]) != _bits(dl))[:5])
        assert _same(tr["dk"][p0:p0 + npair], dk), (r, A, np.flatnonzero(_bits(tr["dk"][p0:p0 + npair]) != _bits(dk))[:5])
        if A >= 2:
            assert _same(tr["height_l"][f:f + A - 1], oracle_lib.hclust_average(A, dl.copy(), which=src)[1]), (r, A)
            assert _same(tr["height_k"][f:f + A - 1], oracle_lib.hclust_average(A, dk.copy(), which=src)[1]), (r, A)
        p0 += npair
    assert saw_nan and p0 == tr["dl"].size
