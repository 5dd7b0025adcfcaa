"""The tag merge model of DESIGN 4.20 restated by brute force (test oracle for mipgen_accel_reads_set_tag_mismatches / _last_tag_merge / _tag_map_fetch and
`mipgen_count -tag_mismatches 1`): raw groups are Python dicts keyed (row, probe, tag bytes), every pair of tags of a cell is compared by plain loops, parents are
followed link by link.  Assignment, samples and the vote are those of reads_ref, samples_ref and consensus_ref.  No sort, no windows, no lanes.  Test infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import consensus_ref as CR
from tests import reads_ref as R
from tests import samples_ref as SR

MAX_LINKS = 31


def one_base_apart(a: int, b: int, n_bases: int) -> bool:
    """Two tag codes of n_bases bases differ in exactly one base."""
    return sum(1 for i in range(n_bases) if ((a >> (2 * i)) & 3) != ((b >> (2 * i)) & 3)) == 1


def eligible(c_parent: int, c_child: int) -> bool:
    return c_parent >= 2 * c_child - 1 and c_parent > c_child


def parents_of_cell(counts: Dict[int, int], n_bases: int) -> Dict[int, Optional[int]]:
    """counts: tag code -> family of the raw groups of ONE cell.  The parent code of every tag, or None for a root."""
    out: Dict[int, Optional[int]] = {}
    for b, cb in counts.items():
        best = None
        for a, ca in counts.items():
            if a == b or not one_base_apart(a, b, n_bases) or not eligible(ca, cb):
                continue
            if best is None or ca > counts[best] or (ca == counts[best] and a < best):
                best = a
        out[b] = best
    return out


def roots_of_cell(counts: Dict[int, int], n_bases: int) -> Dict[int, Tuple[int, int]]:
    """tag code -> (root code, links walked to it)."""
    parent = parents_of_cell(counts, n_bases)
    out = {}
    for b in counts:
        at, links = b, 0
        while parent[at] is not None:
            at = parent[at]; links += 1
            assert links <= MAX_LINKS, "counts rise strictly along parent links"
        out[b] = (at, links)
    return out


def merge_groups(raw: Dict[Tuple[int, int], int], n_bases: int):
    """raw: (cell, tag code) -> family.  Returns (tag_map, totals): tag_map one (cell, raw tag, raw family, corrected tag) per raw group ascending by (cell, raw tag);
    totals as mipgen_tag_merge_totals names them."""
    cells: Dict[int, Dict[int, int]] = {}
    for (cell, code), f in raw.items():
        cells.setdefault(cell, {})[code] = f
    tag_map, absorbed, moved, deepest = [], 0, 0, 0
    for cell in sorted(cells):
        roots = roots_of_cell(cells[cell], n_bases)
        for code in sorted(cells[cell]):
            root, links = roots[code]
            tag_map.append((cell, code, cells[cell][code], root))
            if links:
                absorbed += 1; moved += cells[cell][code]
            deepest = max(deepest, links)
    n_raw = len(raw)
    return tag_map, {"raw_groups": n_raw, "groups": n_raw - absorbed, "absorbed": absorbed, "moved_pairs": moved, "max_depth": deepest}


def consensus_reads(arms, ext_reads, lig_reads, ext_quals, lig_quals, index_reads: Optional[Sequence[bytes]] = None, barcodes: Optional[Sequence[bytes]] = None,
                    barcode_mismatches: int = 0, tag_sizes=(5, 0), mismatches: int = 0, tag_mismatches: int = 1):
    """consensus_ref.consensus_reads with the merge: (reads, unique_tags, totals, row_pairs or None, groups, sample or None, probe, tag_map, merge totals); groups are
    the CORRECTED groups, (cell, root tag code, summed family, ext_seq, ext_qual, lig_seq, lig_qual) ascending by (cell, root tag code); unique_tags counts them."""
    assert tag_mismatches in (0, 1)
    te, tl = tag_sizes
    T = te + tl
    assert T > 0
    n = len(arms)
    if barcodes is None:
        reads, unique, totals, probe = R.count_reads(arms, ext_reads, lig_reads, tag_sizes, mismatches)
        reads, row_pairs, sample = reads[None, :], None, None
        row_of = [0] * len(probe)
    else:
        reads, unique, totals, row_pairs, sample, probe = SR.count_reads_samples(arms, ext_reads, lig_reads, index_reads, barcodes, barcode_mismatches, tag_sizes, mismatches)
        row_of = [int(s) if s >= 0 else len(barcodes) for s in sample]
    members: Dict[Tuple[int, int], List[int]] = {}
    for i, p in enumerate(probe):
        if p < 0:
            continue
        tag = ext_reads[i][:te] + lig_reads[i][:tl]
        if all(c in R.ACGT for c in tag):                            # a dirty tag joins nothing
            members.setdefault((row_of[i] * n + int(p), CR.tag_code(tag)), []).append(i)
    raw = {k: len(m) for k, m in members.items()}
    if tag_mismatches:
        tag_map, merge_totals = merge_groups(raw, T)
    else:
        tag_map = [(cell, code, raw[(cell, code)], code) for cell, code in sorted(raw)]
        merge_totals = {"raw_groups": len(raw), "groups": len(raw), "absorbed": 0, "moved_pairs": 0, "max_depth": 0}
    corrected: Dict[Tuple[int, int], List[int]] = {}
    for cell, code, _, root in tag_map:
        corrected.setdefault((cell, root), []).extend(members[(cell, code)])
    groups = []
    unique = np.zeros(reads.shape, dtype=np.int64)
    for cell, root in sorted(corrected):
        m = corrected[(cell, root)]
        es, eq = CR.collapse([ext_reads[i] for i in m], [ext_quals[i] for i in m], te)
        ls, lq = CR.collapse([lig_reads[i] for i in m], [lig_quals[i] for i in m], tl)
        groups.append((cell, root, len(m), es, eq, ls, lq))
        unique[cell // n, cell % n] += 1
    return reads, unique, totals, row_pairs, groups, sample, probe, tag_map, merge_totals


# ---- what `mipgen_count -tag_mismatches 1 -tag_map FILE` writes ------------------------------------------------------------------------------------------
def tag_map_file(tag_map, keys: Sequence[str], tag_bases: int, labels: Optional[Sequence[str]] = None) -> bytes:
    """One line per raw group in raw group order: sample (as the consensus header writes it), mip_key, raw_tag, raw_family, tag."""
    n = len(keys)
    lines = ["sample\tmip_key\traw_tag\traw_family\ttag\n"]
    for cell, raw_tag, raw_family, tag in tag_map:
        row, p = divmod(cell, n)
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        lines.append(f"{sample}\t{keys[p]}\t{CR.tag_string(raw_tag, tag_bases)}\t{raw_family}\t{CR.tag_string(tag, tag_bases)}\n")
    return "".join(lines).encode()


def stderr_line(t: dict) -> str:
    return f"mipgen_count: tag_mismatches 1 raw {t['raw_groups']} groups {t['groups']} absorbed {t['absorbed']} moved_pairs {t['moved_pairs']} max_depth {t['max_depth']}\n"
