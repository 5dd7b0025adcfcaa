"""The insertion alleles of DESIGN 4.16 restated by brute force (test oracle for mipgen_accel_reads_consensus_insertions, gap_traceback_runs of gapped_align.h and
`mipgen_count -pileup FILE -pileup_indels W -pileup_insertions INS`): plain loops over the path gapped_ref.align returns for every (molecule, side), a string per
event, a dictionary of alleles.  No projection, no packed run index; the 64-bit key is computed only to put the finished alleles in order.  Test infrastructure."""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import gapped_ref as G
from tests import pileup_ref as PR

EXT, LIG = G.EXT, G.LIG
SPAN, INS, INS_DISCORDANT, AMBIGUOUS = 0, 1, 2, 3
MAX_SPELLED = 15                                                        # a longer run is always ambiguous
RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("count", "<i4"), ("bases", "<u4"), ("ambiguous", "<i4")])
TOTAL_KEYS = ("groups", "used", "span", "insertions", "ins_discordant", "ambiguous", "alleles", "gapped_sides")
FILE_HEADER = ">sample\tmip_key\tchr\tposition\tstrand\tlength\tinserted\tcount\tspan\tppm\n"


def side_runs(q: bytes, M: bytes, W: int, side: int) -> Dict[int, Tuple[int, int]]:
    """{anchor t: (insertion length, read index of the run's first base)} for the anchors the side covers, in the orientation of M.  The read index counts every
    read base the path consumed before the run, the insertion steps in front of the first column included."""
    L = len(M)
    if len(q) == 0:
        return {}
    r = M if side == EXT else G.revcomp(M)
    _ie, je, _h, path = G.align(q, r, W, side)
    t_of = (lambda j: j - 1) if side == EXT else (lambda j: L - j)
    i = j = 0
    runs = {}                                                           # column j -> [length, read index]: the run between column j and column j + 1
    for step in path:
        if step == "M":
            i += 1; j += 1
        elif step == "D":
            j += 1
        else:
            if j not in runs:
                runs[j] = [0, i]
            runs[j][0] += 1
            i += 1
    out = {}
    for c in range(1, je):                                              # columns c and c + 1 are both consumed
        length, at = runs.get(c, (0, 0))
        out[min(t_of(c), t_of(c + 1))] = (length, at)
    return out


def side_string(q: bytes, qual: bytes, side: int, at: int, l: int) -> List[Tuple[int, int]]:
    """The l (base byte, quality byte) of a side's run in the orientation of M."""
    if side == EXT:
        return [(q[at + j], qual[at + j]) for j in range(l)]
    return [(PR.COMPLEMENT.get(q[at + l - 1 - j], q[at + l - 1 - j]), qual[at + l - 1 - j]) for j in range(l)]


def event_string(strings: Sequence[List[Tuple[int, int]]], l: int, min_quality: int) -> Optional[bytes]:
    """The inserted bases of a molecule from the strings of its one or two contributing sides, or None if any base is ambiguous."""
    if l > MAX_SPELLED:
        return None
    out = bytearray()
    for j in range(l):
        usable = [b for b, qv in (s[j] for s in strings) if b in G.ACGT and qv - 33 >= min_quality]
        if not usable or any(b != usable[0] for b in usable):
            return None
        out.append(usable[0])
    return bytes(out)


def pack(bases: bytes) -> int:
    v = 0
    for b in bases:
        v = v * 4 + G.ACGT.index(b)
    return v


def unpack(bases: int, l: int) -> bytes:
    return bytes(G.ACGT[(bases >> (2 * (l - 1 - j))) & 3] for j in range(l))


def key(x: int, l: int, ambiguous: bool, bases: int) -> int:
    if l > MAX_SPELLED:
        return x << 35 | 1 << 30 | l
    return x << 35 | l << 31 | int(ambiguous) << 30 | (0 if ambiguous else bases)


def insertions(groups, mol_seq: Sequence[bytes], n: int, row: int, min_family: int = 1, min_quality: int = 0, W: int = 8):
    """(anchors[sum(len M_p)][4] int32 - span, ins, ins_discordant, ambiguous -, the records as an array of RECORD_DTYPE in ascending key order, totals) of the groups
    (cell, tag, family, ext_seq, ext_qual, lig_seq, lig_qual) whose cell lies in `row`."""
    assert len(mol_seq) == n and all(len(M) >= 1 for M in mol_seq) and 1 <= W <= 15
    pos_off = [sum(len(M) for M in mol_seq[:p]) for p in range(n)]
    anchors = np.zeros((sum(len(M) for M in mol_seq), 4), dtype=np.int32)
    alleles: Dict[Tuple[int, int, Optional[bytes]], int] = {}
    totals = dict.fromkeys(TOTAL_KEYS, 0)
    for cell, _tag, family, es, eq, ls, lq in groups:
        if cell // n != row:
            continue
        totals["groups"] += 1
        if family < min_family:
            continue
        totals["used"] += 1
        p = cell % n
        M = mol_seq[p]
        sides = ((es, eq, EXT), (ls, lq, LIG))
        runs = [side_runs(q, M, W, side) for q, _qual, side in sides]
        totals["gapped_sides"] += sum(G.side_view(q, qual, M, W, side)[2] > 0 for q, qual, side in sides)
        for t in range(len(M) - 1):
            cover = [(k, runs[k][t]) for k in range(2) if t in runs[k]]
            if not cover:
                continue
            x = pos_off[p] + t
            lengths = {length for _k, (length, _at) in cover}
            if len(lengths) > 1:
                anchors[x][INS_DISCORDANT] += 1
                continue
            l = lengths.pop()
            anchors[x][SPAN] += 1
            if l == 0:
                continue
            anchors[x][INS] += 1
            s = event_string([side_string(sides[k][0], sides[k][1], sides[k][2], at, l) for k, (_l, at) in cover], l, min_quality)
            if s is None:
                anchors[x][AMBIGUOUS] += 1
            alleles[(x, l, s)] = alleles.get((x, l, s), 0) + 1
    ordered = sorted(alleles.items(), key=lambda a: key(a[0][0], a[0][1], a[0][2] is None, 0 if a[0][2] is None else pack(a[0][2])))
    records = np.zeros(len(ordered), dtype=RECORD_DTYPE)
    for k, ((x, l, s), count) in enumerate(ordered):
        records[k] = (x, l, count, 0 if s is None else pack(s), int(s is None))
    totals.update(span=int(anchors[:, SPAN].sum()), insertions=int(anchors[:, INS].sum()), ins_discordant=int(anchors[:, INS_DISCORDANT].sum()),
                  ambiguous=int(anchors[:, AMBIGUOUS].sum()), alleles=len(ordered))
    return anchors, records, totals


# ---- what `mipgen_count ... -pileup_insertions INS` writes ---------------------------------------------------------------------------------------------------
def record_line(fields: Sequence[bytes], t: int, record, span: int) -> Tuple[int, str, str]:
    """(position, strand, inserted) of a record at anchor t of the probe whose table row is `fields`: the position is the lower genome coordinate of the anchor's
    two neighbours t and t + 1; the inserted bases are reverse-complemented on a minus probe; an ambiguous record prints N."""
    l = int(record["length"])
    inserted = b"N" * l if record["ambiguous"] else unpack(int(record["bases"]), l)
    if fields[17] == b"+":
        return int(fields[3]) + t, "+", inserted.decode()
    return int(fields[4]) - (t + 1), "-", G.revcomp(inserted).decode()


def insertions_file(groups, table_rows: Sequence[Sequence[bytes]], labels: Optional[Sequence[str]] = None, min_family: int = 1, min_quality: int = 0,
                    W: int = 8) -> Tuple[bytes, str]:
    """(the -pileup_insertions file, its stderr line): one line per record, in row order, then table row order, then record order."""
    n = len(table_rows)
    mol_seq = [(f[6] + f[13] + f[10]).upper() for f in table_rows]
    pos_off = [sum(len(M) for M in mol_seq[:p]) for p in range(n)]
    n_rows = 1 if labels is None else len(labels) + 1
    out = [FILE_HEADER]
    n_alleles = events = ambiguous = span_total = 0
    for row in range(n_rows):
        anchors, records, totals = insertions(groups, mol_seq, n, row, min_family, min_quality, W)
        n_alleles += totals["alleles"]; events += totals["insertions"]; ambiguous += totals["ambiguous"]; span_total += totals["span"]
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        for rec in records:                                             # (ascending key: ascending position, so table row order)
            x = int(rec["pos"])
            p = max(k for k in range(n) if pos_off[k] <= x)
            f = table_rows[p]
            span = int(anchors[x][SPAN])
            pos, strand, inserted = record_line(f, x - pos_off[p], rec, span)
            out.append(f"{sample}\t{f[0].decode()}\t{f[2].decode()}\t{pos}\t{strand}\t{int(rec['length'])}\t{inserted}\t{int(rec['count'])}\t{span}\t"
                       f"{int(rec['count']) * 1000000 // span}\n")
    line = f"mipgen_count: insertion alleles {n_alleles} events {events} ambiguous {ambiguous} span {span_total}\n"
    return "".join(out).encode(), line
