"""The capture model of DESIGN 4.9 restated by brute force (test oracle for mipgen_accel_reads_* and `mipgen_count`): every read pair is compared
against every probe - no seeds table, no hashing, no cap on candidates, no chunks - and tag groups are Python sets.  It can agree with the device
only if the device's short-cuts (seed lookups, the union of the two ranges, the chunked sort-unique) are exact.  Test infrastructure."""
from typing import Dict, List, Sequence, Tuple

import numpy as np

_COMP = {ord("A"): ord("T"), ord("C"): ord("G"), ord("G"): ord("C"), ord("T"): ord("A")}
ACGT = frozenset(b"ACGT")
MAX_SEED = 32
UNASSIGNED, AMBIGUOUS = -1, -2


def revcomp(s: bytes) -> bytes:
    """Reverse complement of upper-case A C G T; every other byte becomes 'N' (which matches nothing)."""
    return bytes(_COMP.get(c, ord("N")) for c in reversed(s))


def seed_length(arms: Sequence[Tuple[bytes, bytes]]) -> int:
    return min(MAX_SEED, min(min(len(e), len(l)) for e, l in arms))


def _matrix(reads: Sequence[bytes], skip: int, width: int):
    """Bytes [skip, skip + width) of every read as a matrix, 0 where the read has ended, and the number of bases each read has after `skip`."""
    m = np.zeros((len(reads), width), dtype=np.uint8)
    avail = np.zeros(len(reads), dtype=np.int64)
    for i, r in enumerate(reads):
        t = r[skip:skip + width]
        m[i, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        avail[i] = max(len(r) - skip, 0)
    return m, avail


def _arm_equal(m: np.ndarray, arm: bytes) -> np.ndarray:
    """[pair][base]: the read's base equals the arm's base and both are upper-case A C G T."""
    a = np.frombuffer(arm, dtype=np.uint8)
    ok = np.isin(a, np.frombuffer(b"ACGT", dtype=np.uint8))
    return (m[:, :len(a)] == a[None, :]) & ok[None, :]


def assign_reads(arms: Sequence[Tuple[bytes, bytes]], ext_reads: Sequence[bytes], lig_reads: Sequence[bytes], tag_sizes=(5, 0), mismatches: int = 0) -> np.ndarray:
    """Probe index per pair, UNASSIGNED or AMBIGUOUS."""
    te, tl = tag_sizes
    S = seed_length(arms)
    assert S >= 12 and 0 <= mismatches <= 2 and te + tl <= 16
    width = max(max(len(e), len(l)) for e, l in arms)
    X, avail_e = _matrix(ext_reads, te, width)
    Y, avail_l = _matrix(lig_reads, tl, width)
    n = len(ext_reads)
    best = np.full(n, 1 << 30, dtype=np.int64)
    best_p = np.full(n, UNASSIGNED, dtype=np.int64)
    ties = np.zeros(n, dtype=np.int64)
    for p, (E, L) in enumerate(arms):
        R = revcomp(L)
        eq_e, eq_l = _arm_equal(X, E), _arm_equal(Y, R)
        candidate = (eq_e[:, :S].all(axis=1) & (avail_e >= S)) | (eq_l[:, :S].all(axis=1) & (avail_l >= S))
        me, ml = len(E) - eq_e.sum(axis=1), len(R) - eq_l.sum(axis=1)
        passes = candidate & (avail_e >= len(E)) & (avail_l >= len(R)) & (me <= mismatches) & (ml <= mismatches)
        tot = me + ml
        better = passes & (tot < best)
        tie = passes & (tot == best)
        best[better] = tot[better]; best_p[better] = p; ties[better] = 1
        ties[tie] += 1
    out = best_p.copy()
    out[ties > 1] = AMBIGUOUS
    return out


def count_reads(arms: Sequence[Tuple[bytes, bytes]], ext_reads: Sequence[bytes], lig_reads: Sequence[bytes], tag_sizes=(5, 0), mismatches: int = 0,
                swap_reads: bool = False):
    """(reads, unique_tags, totals, assignment) of the model."""
    if swap_reads:
        ext_reads, lig_reads = lig_reads, ext_reads
    te, tl = tag_sizes
    a = assign_reads(arms, ext_reads, lig_reads, tag_sizes, mismatches)
    reads = np.zeros(len(arms), dtype=np.int64)
    groups: List[set] = [set() for _ in arms]
    tag_n = 0
    for i, p in enumerate(a):
        if p < 0:
            continue
        reads[p] += 1
        tag = ext_reads[i][:te] + lig_reads[i][:tl]
        if all(c in ACGT for c in tag):
            groups[p].add(tag)
        else:
            tag_n += 1
    unique = reads.copy() if te + tl == 0 else np.array([len(g) for g in groups], dtype=np.int64)
    totals: Dict[str, int] = {"pairs": len(a), "assigned": int((a >= 0).sum()), "ambiguous": int((a == AMBIGUOUS).sum()),
                              "unassigned": int((a == UNASSIGNED).sum()), "tag_n": tag_n, "overflow": 0}
    return reads, unique, totals, a.astype(np.int32)


def counts_tsv(keys_names: Sequence[Tuple[str, str]], reads: np.ndarray, unique: np.ndarray) -> bytes:
    """What `mipgen_count -o` writes."""
    rows = ["mip_key\tmip_name\treads\tunique_tags"] + [f"{k}\t{nm}\t{int(r)}\t{int(u)}" for (k, nm), r, u in zip(keys_names, reads, unique)]
    return ("\n".join(rows) + "\n").encode()
