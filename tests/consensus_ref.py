"""The consensus model of DESIGN 4.11 restated by brute force (test oracle for mipgen_accel_reads_*_consensus and `mipgen_count -consensus`): groups are
Python dicts keyed (row, probe, tag bytes), the vote is a plain loop over members and positions, every probe comes through reads_ref.assign_reads and
every sample through samples_ref.  No sort, no chunks, no lanes.  Test infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

from tests import reads_ref as R
from tests import samples_ref as SR

CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def quality_of(byte: int) -> int:
    return min(max(byte - 33, 0), 93)


def call_position(votes: Sequence[Tuple[int, int]]) -> Tuple[int, int]:
    """(base byte, quality byte) of one position from the (base byte, quality byte) of every member there."""
    S = {b: 0 for b in b"ACGT"}
    for base, qual in votes:
        if base in S:                                                # any other byte casts no vote
            S[base] += quality_of(qual)
    top = max(S.values())
    best = [b for b in b"ACGT" if S[b] == top]
    total = sum(S.values())
    if top == 0 or len(best) > 1:
        base, v = ord("N"), -total
    else:
        base, v = best[0], top - (total - top)
    return base, ord("I") if v > 40 else ord("#") if v < 2 else v + 33


def collapse(reads: Sequence[bytes], quals: Sequence[bytes], skip: int) -> Tuple[bytes, bytes]:
    """One side of a group: the reads of its members behind `skip` tag bases, as long as the shortest of them."""
    length = min(max(len(r) - skip, 0) for r in reads)
    seq, qual = bytearray(), bytearray()
    for j in range(length):
        b, q = call_position([(r[skip + j], s[skip + j]) for r, s in zip(reads, quals)])
        seq.append(b); qual.append(q)
    return bytes(seq), bytes(qual)


def tag_code(tag: bytes) -> int:
    """The 2-bit code of a clean tag, its first base highest."""
    code = 0
    for c in tag:
        code = (code << 2) | CODE[c]
    return code


def consensus_reads(arms, ext_reads, lig_reads, ext_quals, lig_quals, index_reads: Optional[Sequence[bytes]] = None, barcodes: Optional[Sequence[bytes]] = None,
                    barcode_mismatches: int = 0, tag_sizes=(5, 0), mismatches: int = 0, swap_reads: bool = False):
    """(reads[rows][n], unique_tags[rows][n], totals, row_pairs or None, groups, sample_index or None, probe_index) of the model.  groups: a list of
    (cell, tag code, family, ext_seq, ext_qual, lig_seq, lig_qual) ascending by (row, probe, tag code); cell = row * n + probe."""
    if swap_reads:
        ext_reads, lig_reads, ext_quals, lig_quals = lig_reads, ext_reads, lig_quals, ext_quals
    te, tl = tag_sizes
    assert te + tl > 0 and all(len(r) == len(q) for r, q in zip(list(ext_reads) + list(lig_reads), list(ext_quals) + list(lig_quals)))
    n = len(arms)
    if barcodes is None:
        reads, unique, totals, probe = R.count_reads(arms, ext_reads, lig_reads, tag_sizes, mismatches)
        reads, unique, row_pairs, sample = reads[None, :], unique[None, :], None, None
        row_of = [0] * len(probe)
    else:
        reads, unique, totals, row_pairs, sample, probe = SR.count_reads_samples(arms, ext_reads, lig_reads, index_reads, barcodes, barcode_mismatches, tag_sizes, mismatches)
        row_of = [int(s) if s >= 0 else len(barcodes) for s in sample]
    members: Dict[Tuple[int, int, bytes], List[int]] = {}
    for i, p in enumerate(probe):
        if p < 0:
            continue
        tag = ext_reads[i][:te] + lig_reads[i][:tl]
        if all(c in R.ACGT for c in tag):
            members.setdefault((row_of[i], int(p), tag), []).append(i)
    groups = []
    for (row, p, tag) in sorted(members, key=lambda k: (k[0], k[1], tag_code(k[2]))):
        m = members[(row, p, tag)]
        es, eq = collapse([ext_reads[i] for i in m], [ext_quals[i] for i in m], te)
        ls, lq = collapse([lig_reads[i] for i in m], [lig_quals[i] for i in m], tl)
        groups.append((row * n + p, tag_code(tag), len(m), es, eq, ls, lq))
    return reads, unique, totals, row_pairs, groups, sample, probe


# ---- what `mipgen_count -consensus` writes ---------------------------------------------------------------------------------------------------------
def tag_string(code: int, n_bases: int) -> str:
    return "".join("ACGT"[(code >> (2 * (n_bases - 1 - j))) & 3] for j in range(n_bases))


def consensus_fastq(groups, keys: Sequence[str], tag_bases: int, labels: Optional[Sequence[str]] = None, min_family: int = 1) -> Tuple[bytes, bytes, str]:
    """(PREFIX.ext.fq, PREFIX.lig.fq, the stderr line): one record per group of at least min_family members, in group order; the ordinal is the group's
    place in the list of ALL groups, from 0 (it does not depend on min_family); `members` is over every group."""
    n = len(keys)
    ext, lig = [], []
    written = 0
    for g, (cell, tag, family, es, eq, ls, lq) in enumerate(groups):
        if family < min_family:
            continue
        row, p = divmod(cell, n)
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        head = f"@smc{g} {sample}\t{keys[p]}\t{tag_string(tag, tag_bases)}\t{family}\n".encode()
        ext.append(head + es + b"\n+\n" + eq + b"\n")
        lig.append(head + ls + b"\n+\n" + lq + b"\n")
        written += 1
    line = f"mipgen_count: consensus groups {len(groups)} written {written} members {sum(g[2] for g in groups)}\n"
    return b"".join(ext), b"".join(lig), line
