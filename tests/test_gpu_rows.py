"""GPU: the rows an allele operator is given (an arena plus seq_off / seq_len), over the five batch methods: a row outside the arena is
refused by the entry's own name before anything runs, a call without alleles (unit alignment and unit parse: without tasks) succeeds with
empty results of the documented shapes, and the alleles of a motif call stay on the device for unitalign_motifs across a refused motif
call and across a unit alignment of other alleles.

Three alleles: (CAG)8, (ACGT)5 and the empty one.  The empty one stands last: the row moved to the arena's last byte must have bases to lie
outside it (an empty row there lies inside)."""
import re
import numpy as np
import pytest
from otter_amd import abi
from otter_amd._lib import OtterGpuError

pytestmark = pytest.mark.gpu
SEQS = [b"CAG" * 8, b"ACGT" * 5, b""]
UNITS = [b"CAG", b"ACGT"]

# name, entry, the call on (gpu, arena, off, ln, with_tasks), the empty results as (shape, dtype) per returned array
OPS = [
    ("kmer_usage", "otg_kmer_usage_batch", lambda g, a, o, l, t: g.kmer_usage_batch(a, o, l, k=3),
     [((0, 65), np.float64), ((0,), np.float64), ((0,), np.float64)]),
    ("motif", "otg_motif_batch", lambda g, a, o, l, t: g.motif_batch(a, o, l),
     [((0,), abi.motif_dt), ((0, 1), np.uint8)]),
    ("repeat", "otg_repeat_batch", lambda g, a, o, l, t: g.repeat_batch(a, o, l),
     [((0,), abi.repeat_sum_dt), ((1,), np.uint64), ((0,), abi.repeat_seg_dt)]),
    ("unitalign", "otg_unitalign_batch", lambda g, a, o, l, t: g.unitalign_batch(a, o, l, UNITS, [0, 1][:t], [0, 1][:t]),
     [((0,), abi.unitalign_dt)]),
    ("unitparse", "otg_unitparse_batch", lambda g, a, o, l, t: g.unitparse_batch(a, o, l, [UNITS], [0, 1][:t], [0, 0][:t]),
     [((0,), abi.unitparse_sum_dt), ((1,), np.uint64), ((0,), abi.unitparse_seg_dt)]),
]
IDS = [op[0] for op in OPS]


def _outside():
    """the three alleles with the second one moved to the last byte of the arena"""
    arena, off, ln = abi.pack_seqs(SEQS)
    off = off.copy()
    off[1] = arena.size - 1
    return arena, off, ln


@pytest.mark.parametrize("name,entry,call,empty", OPS, ids=IDS)
def test_offset_outside_the_arena(gpu, name, entry, call, empty):
    arena, off, ln = _outside()
    with pytest.raises(OtterGpuError) as e:
        call(gpu, arena, off, ln, 2)
    want = "%s failed (%d): %s: allele 1 (offset %d, length %d) lies outside the %d-byte arena" % (
        entry, abi.OTG_ERR_ARG, entry, arena.size - 1, len(SEQS[1]), arena.size)
    assert str(e.value) == want


@pytest.mark.parametrize("name,entry,call,empty", OPS, ids=IDS)
def test_zero_alleles(gpu, name, entry, call, empty):
    if name in ("unitalign", "unitparse"):                                  # alleles and units, no task
        res = call(gpu, *abi.pack_seqs(SEQS), 0)
    else:
        res = call(gpu, *abi.pack_seqs([]), 0)
    res = res if isinstance(res, tuple) else (res,)
    assert len(res) == len(empty)
    for got, (shape, dtype) in zip(res, empty):
        assert got.shape == shape and got.dtype == dtype, (name, got.shape, got.dtype)
        assert not any(got.tobytes())                                       # (seg_off of no rows is [0])


_FIRST = []


def _first_call_alone(gpu):
    """the records of unitalign_motifs right behind motif_batch on the three alleles"""
    if not _FIRST:
        gpu.motif_batch(*abi.pack_seqs(SEQS))
        _FIRST.append(gpu.unitalign_motifs())
        rec = _FIRST[0]
        assert rec.shape == (3,)
        # a perfect repeat is its own unit's copies: no edit, every base a unit base; the empty allele has no unit
        assert (int(rec[0]["edits"]), int(rec[0]["unit_bases"]), int(rec[0]["flags"])) == (0, 24, 0)
        assert (int(rec[1]["edits"]), int(rec[1]["unit_bases"]), int(rec[1]["flags"])) == (0, 20, 0)
        assert int(rec[2]["flags"]) == abi.UNITALIGN_NO_UNIT
    return _FIRST[0]


def test_alleles_of_a_motif_call_survive_a_refused_one(gpu):
    want = _first_call_alone(gpu)
    gpu.motif_batch(*abi.pack_seqs(SEQS))
    with pytest.raises(OtterGpuError, match=re.escape("lies outside")):
        gpu.motif_batch(*_outside())
    assert gpu.unitalign_motifs().tobytes() == want.tobytes()


def test_alleles_of_a_motif_call_survive_a_unit_alignment_of_others(gpu):
    want = _first_call_alone(gpu)
    gpu.motif_batch(*abi.pack_seqs(SEQS))
    others = [b"GATTACA" * 9, b"T" * 50, b"AC" * 40]                          # longer than the motif call's arena
    rec = gpu.unitalign_batch(*abi.pack_seqs(others), [b"GATTACA", b"AC"], [0, 1, 2], [0, 1, 1])
    assert (int(rec[0]["edits"]), int(rec[0]["unit_bases"])) == (0, 63) and (int(rec[2]["edits"]), int(rec[2]["unit_bases"])) == (0, 80)
    assert gpu.unitalign_motifs().tobytes() == want.tobytes()
