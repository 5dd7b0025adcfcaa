"""The insertion calls of DESIGN 4.17 restated by brute force (test oracle for mipgen_accel_insertion_call_tables, mipgen_accel_reads_consensus_insertion_pool /
_insertion_call and `mipgen_count -call_insertions`): plain loops and dictionaries over what tests/insertion_ref.py gives per row.  A row is a dictionary
allele -> (k, n); the background of an allele is summed over the sample rows one by one, each asked whether it qualifies - no sorted array, no search, no
S - X.  The filters, the leave-one-out and the score are imported from tests/call_ref.py, not restated.  Test infrastructure."""
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import call_ref as CR
from tests import insertion_ref as I

POOL_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("bases", "<u4"), ("bg_alt", "<i4"), ("bg_excluded", "<i4")])
CALL_RECORD_DTYPE = np.dtype([("pos", "<i8"), ("length", "<i4"), ("bases", "<u4"), ("depth", "<i4"), ("alt", "<i4"), ("bg_alt", "<i4"), ("bg_depth", "<i4"), ("q", "<i4"),
                              ("reserved", "<i4")])
FILE_HEADER = ">sample\tmip_key\tchr\tposition\tstrand\tlength\tinserted\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\n"
Allele = Tuple[int, int, int]                                            # (pos, length, bases)


class Row:
    """What a row shows: span per anchor and the count of every non-ambiguous allele.  `records` keeps the row's record array (ambiguous ones included) in order."""

    def __init__(self, anchors: np.ndarray, records: np.ndarray):
        self.span = [int(v) for v in (anchors[:, I.SPAN] if anchors.ndim == 2 else anchors)]
        self.records = records
        self.count: Dict[Allele, int] = {}
        for r in records:
            if not r["ambiguous"]:
                a = (int(r["pos"]), int(r["length"]), int(r["bases"]))
                assert a not in self.count and 1 <= a[1] <= I.MAX_SPELLED
                self.count[a] = int(r["count"])


def background(sample_rows: Sequence[Row], a: Allele, bg_max_ppm: int) -> Tuple[int, int]:
    """(K, N) of allele a: k' and n' summed over the sample rows that qualify there."""
    K = N = 0
    for row in sample_rows:
        k, n = row.count.get(a, 0), row.span[a[0]]
        if CR.qualifies(k, n, bg_max_ppm):
            K += k
            N += n
    return K, N


def sparse_pool(sample_rows: Sequence[Row], bg_max_ppm: int) -> Tuple[np.ndarray, np.ndarray]:
    """What mipgen_accel_insertion_pool_fetch owes: (a record per distinct allele of any sample row in ascending key order - bg_alt the k' of the rows that qualify,
    bg_excluded the n' of the rows whose record does not -, S[n_pos] the span summed over all sample rows)."""
    n_pos = len(sample_rows[0].span)
    S = np.zeros(n_pos, dtype=np.int64)
    for row in sample_rows:
        S += np.array(row.span, dtype=np.int64)
    alleles = sorted({a for row in sample_rows for a in row.count}, key=lambda a: I.key(a[0], a[1], False, a[2]))
    out = np.zeros(len(alleles), dtype=POOL_RECORD_DTYPE)
    for i, a in enumerate(alleles):
        K = X = 0
        for row in sample_rows:
            if a in row.count:
                k, n = row.count[a], row.span[a[0]]
                if CR.qualifies(k, n, bg_max_ppm):
                    K += k
                else:
                    X += n
        out[i] = (a[0], a[1], a[2], K, X)
    assert S.max(initial=0) < 2 ** 31
    return out, S.astype(np.int32)


def pool_lookup(pool_records: np.ndarray, pool_span) -> Callable[[Allele], Tuple[int, int]]:
    """The background function of a pool given as mipgen_accel_insertion_call_tables takes it: a dictionary of the records; an absent allele has K = 0, N = S."""
    table = {(int(r["pos"]), int(r["length"]), int(r["bases"])): (int(r["bg_alt"]), int(r["bg_excluded"])) for r in pool_records}

    def bg(a: Allele) -> Tuple[int, int]:
        K, X = table.get(a, (0, 0))
        return K, int(pool_span[a[0]]) - X
    return bg


def call_cells(row: Row, bg: Callable[[Allele], Tuple[int, int]], own_row_is_sample: bool, p: Dict[str, int], score=CR.exact_phred, filters_only: bool = False):
    """(totals dict, candidates) of one row, as call_ref.call_cells gives them: every candidate a dict of the call record's fields plus phred, excluded, q; in record
    order, which is ascending allele key."""
    totals = {"tested": 0, "too_deep": 0, "candidates": 0, "calls": 0, "excluded": 0}
    out = []
    for r in row.records:
        if r["ambiguous"]:
            continue
        a = (int(r["pos"]), int(r["length"]), int(r["bases"]))
        k, n = int(r["count"]), row.span[a[0]]
        assert n >= k >= 1
        if n > CR.MAX_DEPTH:
            totals["too_deep"] += 1
            continue
        if n < p["min_depth"]:
            continue
        totals["tested"] += 1
        K, N = bg(a)
        K_o, N_o = CR.leave_one_out(K, N, k, n, own_row_is_sample, p["bg_max_ppm"])
        if not CR.candidate(k, n, K_o, N_o, p):
            continue
        totals["candidates"] += 1
        rec = {"pos": a[0], "length": a[1], "bases": a[2], "depth": n, "alt": k, "bg_alt": K_o, "bg_depth": N_o, "phred": None, "excluded": False, "q": None}
        if not filters_only:
            rec["phred"] = score(k, n, K_o + p["a0"], N_o + p["n0"])
            rec["excluded"] = CR.near_integer(rec["phred"])
            rec["q"] = CR.q_of(rec["phred"])
            totals["excluded"] += rec["excluded"]
            totals["calls"] += (not rec["excluded"]) and rec["q"] >= p["min_q"]
        out.append(rec)
    return totals, out


def kept_calls(cands: Sequence[dict], p: Dict[str, int]) -> List[tuple]:
    """The records the device owes: the candidates outside the band with q >= min_q, as tuples in the field order of mipgen_insertion_call_record."""
    return [(c["pos"], c["length"], c["bases"], c["depth"], c["alt"], c["bg_alt"], c["bg_depth"], c["q"], 0) for c in cands if not c["excluded"] and c["q"] >= p["min_q"]]


def drop_excluded(records, cands: Sequence[dict]) -> List[tuple]:
    """The device's records without those whose cell the band excludes."""
    banned = {(c["pos"], c["length"], c["bases"]) for c in cands if c["excluded"]}
    return [tuple(int(v) for v in r) for r in records if (int(r[0]), int(r[1]), int(r[2])) not in banned]


def session_rows(groups, mol_seq: Sequence[bytes], n_rows: int, min_family: int = 1, min_quality: int = 0, W: int = 8) -> List[Row]:
    """Every row of a session from its consensus groups, through insertion_ref.insertions."""
    return [Row(*I.insertions(groups, mol_seq, len(mol_seq), row, min_family, min_quality, W)[:2]) for row in range(n_rows)]


def call_session(rows: Sequence[Row], barcodes: bool, p: Dict[str, int], score=CR.exact_phred):
    """[(totals, candidates)] per row of a session: the sample rows are all rows but the last when it has barcodes, the one row otherwise."""
    n_sample = len(rows) - 1 if barcodes else 1
    samples = rows[:n_sample]
    return [call_cells(row, lambda a: background(samples, a, p["bg_max_ppm"]), r < n_sample, p, score) for r, row in enumerate(rows)]


# ---- what `mipgen_count ... -call_insertions ICALLS` writes ----------------------------------------------------------------------------------------------------
def calls_file(groups, table_rows: Sequence[Sequence[bytes]], labels: Optional[Sequence[str]], p: Dict[str, int], min_family: int = 1, min_quality: int = 0,
               W: int = 8) -> Tuple[bytes, str, int]:
    """(the -call_insertions file, its stderr line, candidates excluded by the band): one line per call, in row order, then table row order, then record order."""
    n = len(table_rows)
    mol_seq = [(f[6] + f[13] + f[10]).upper() for f in table_rows]
    pos_off = [sum(len(M) for M in mol_seq[:q]) for q in range(n)]
    rows = session_rows(groups, mol_seq, 1 if labels is None else len(labels) + 1, min_family, min_quality, W)
    out = [FILE_HEADER]
    sums = {"calls": 0, "candidates": 0, "tested": 0, "too_deep": 0, "excluded": 0}
    for r, (totals, cands) in enumerate(call_session(rows, labels is not None, p)):
        sample = "*" if labels is None else labels[r] if r < len(labels) else "undetermined"
        for key in sums:
            sums[key] += totals[key]
        for x, l, bases, depth, k, K_o, N_o, q, _reserved in kept_calls(cands, p):
            i = max(j for j in range(n) if pos_off[j] <= x)
            f = table_rows[i]
            pos, strand, inserted = I.record_line(f, x - pos_off[i], {"length": l, "bases": bases, "ambiguous": 0}, depth)
            out.append(f"{sample}\t{f[0].decode()}\t{f[2].decode()}\t{pos}\t{strand}\t{l}\t{inserted}\t{depth}\t{k}\t{k * CR.MILLION // depth}\t{K_o}\t{N_o}\t{q}\n")
    stderr = f"mipgen_count: insertion calls {sums['calls']} candidates {sums['candidates']} tested {sums['tested']} too_deep {sums['too_deep']}\n"
    return "".join(out).encode(), stderr, sums["excluded"]
