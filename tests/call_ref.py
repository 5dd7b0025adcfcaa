"""The variant-calling model of DESIGN 4.14 restated by brute force (test oracle for mipgen_accel_call_tables, mipgen_accel_reads_consensus_call and
`mipgen_count -call`): plain loops over rows, positions and allele classes, and the binomial tail as an EXACT Python integer: the sum of C(n,i) A^i B^(n-i) over
ALL i = k..n with e = A / (A + B), over (A + B)^n.  No early stop, no log-gamma, no table; -10 log10 comes from math.log10 of the two big integers.  Test
infrastructure."""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_DEPTH = 1 << 20
Q_CAP = 9999
MILLION = 10 ** 6
DELTA = 1e-6                         # the exclusion band around an integer score (and around the cap)
ALLELE_TEXT = "ACGT-"
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
DEFAULTS = dict(min_depth=20, min_alt=3, min_ppm=0, min_q=30, a0=1, n0=1000, bg_max_ppm=200000)


def params(**kw) -> Dict[str, int]:
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def alleles(columns: int) -> int:
    return 5 if columns == 8 else 4


def allele_count(row, columns: int, a: int) -> int:
    return int(row[a]) if a < 4 else int(row[5]) if columns == 8 else 0


def depth(row, columns: int) -> int:
    return int(row[0]) + int(row[1]) + int(row[2]) + int(row[3]) + (int(row[5]) if columns == 8 else 0)


def ref_class(byte: int) -> int:
    return "ACGT".find(chr(byte).upper()) if chr(byte).upper() in "ACGT" else -1


def qualifies(k: int, n: int, bg_max_ppm: int) -> bool:
    return n > 0 and k * MILLION <= bg_max_ppm * n


def pool(tables: Sequence[np.ndarray], bg_max_ppm: int) -> np.ndarray:
    """int32 [n_pos][10], K[5] then N[5] per position, over the tables of the SAMPLE rows."""
    n_pos, columns = tables[0].shape
    out = np.zeros((n_pos, 10), dtype=np.int64)
    for t in tables:
        for x in range(n_pos):
            n = depth(t[x], columns)
            for a in range(5):
                k = allele_count(t[x], columns, a)
                if qualifies(k, n, bg_max_ppm):
                    out[x][a] += k
                    out[x][5 + a] += n
    assert out.max(initial=0) < 2 ** 31
    return out.astype(np.int32)


def leave_one_out(K: int, N: int, k: int, n: int, own_row_is_sample: bool, bg_max_ppm: int) -> Tuple[int, int]:
    if own_row_is_sample and qualifies(k, n, bg_max_ppm):
        return K - k, N - n
    return K, N


def candidate(k: int, n: int, K_o: int, N_o: int, p: Dict[str, int]) -> bool:
    return (p["min_depth"] <= n <= MAX_DEPTH and k >= p["min_alt"] and k * MILLION >= p["min_ppm"] * n and k * (N_o + p["n0"]) > n * (K_o + p["a0"]))


def exact_phred(k: int, n: int, A: int, B: int) -> float:
    """-10 log10 of P(X >= k), X binomial(n, A / B): every term an exact integer, the quotient taken in logarithms of the two big integers."""
    a, b = A, B - A
    assert 0 < a < B and 0 <= k <= n
    term = math.comb(n, k) * a ** k * b ** (n - k)
    total = 0
    for i in range(k, n + 1):
        total += term
        if i < n:
            term = term * (n - i) * a // ((i + 1) * b)                 # C(n,i+1) a^(i+1) b^(n-i-1) from its predecessor: the division is exact
    assert term == a ** n                                              # ... which the last term, known in closed form, confirms for the whole chain
    return -10.0 * (math.log10(total) - n * math.log10(B))


def near_integer(phred: float) -> bool:
    """Within DELTA of an integer at or below the cap - the floor could go either way - and so within DELTA of the cap itself."""
    if phred > Q_CAP + DELTA:
        return False
    return abs(phred - round(phred)) <= DELTA


def q_of(phred: float) -> int:
    return min(Q_CAP, max(0, math.floor(phred)))


def call_cells(counts: np.ndarray, pool_: np.ndarray, ref: bytes, own_row_is_sample: bool, p: Dict[str, int], filters_only: bool = False):
    """(totals dict, candidates): every candidate as a dict of the record's fields plus `phred` (exact, before the floor; None with filters_only or above the depth
    the exact sum is asked for) and `excluded` (near_integer).  Ascending (pos, allele).  totals["calls"] counts candidates with q >= min_q that are not excluded;
    totals["excluded"] says how many the band dropped."""
    n_pos, columns = counts.shape
    totals = {"tested": 0, "too_deep": 0, "candidates": 0, "calls": 0, "excluded": 0}
    out = []
    for x in range(n_pos):
        r = ref_class(ref[x])
        if r < 0:
            continue
        n = depth(counts[x], columns)
        if n > MAX_DEPTH:
            totals["too_deep"] += 1
            continue
        if n < p["min_depth"]:
            continue
        totals["tested"] += 1
        for a in range(alleles(columns)):
            if a == r:
                continue
            k = allele_count(counts[x], columns, a)
            K_o, N_o = leave_one_out(int(pool_[x][a]), int(pool_[x][5 + a]), k, n, own_row_is_sample, p["bg_max_ppm"])
            if not candidate(k, n, K_o, N_o, p):
                continue
            totals["candidates"] += 1
            rec = {"pos": x, "allele": a, "depth": n, "alt": k, "bg_alt": K_o, "bg_depth": N_o, "phred": None, "excluded": False, "q": None}
            if not filters_only:
                rec["phred"] = exact_phred(k, n, K_o + p["a0"], N_o + p["n0"])
                rec["excluded"] = near_integer(rec["phred"])
                rec["q"] = q_of(rec["phred"])
                totals["excluded"] += rec["excluded"]
                totals["calls"] += (not rec["excluded"]) and rec["q"] >= p["min_q"]
            out.append(rec)
    return totals, out


def kept_calls(cands: Sequence[dict], p: Dict[str, int]) -> List[tuple]:
    """The records the device owes: the candidates outside the band with q >= min_q, as tuples in the field order of mipgen_call_record."""
    return [(c["pos"], c["allele"], c["depth"], c["alt"], c["bg_alt"], c["bg_depth"], c["q"]) for c in cands if not c["excluded"] and c["q"] >= p["min_q"]]


def drop_excluded(records, cands: Sequence[dict]) -> List[tuple]:
    """The device's records without those whose cell the band excludes."""
    banned = {(c["pos"], c["allele"]) for c in cands if c["excluded"]}
    return [tuple(int(v) for v in r) for r in records if (int(r[0]), int(r[1])) not in banned]


# ---- what `mipgen_count -call` writes ------------------------------------------------------------------------------------------------------------------------
CALLS_HEADER = ">sample\tmip_key\tchr\tposition\tstrand\tpart\tref\talt\tdepth\talt_count\talt_ppm\tbg_alt\tbg_depth\tq\n"


def call_line(sample: str, fields: Sequence[bytes], t: int, rec: tuple) -> Tuple[int, str]:
    """(the rank of the printed alt within its position, the line) of one record at template position t of the table row `fields` (its 20 columns as bytes)."""
    E, T, L = fields[6], fields[13], fields[10]
    M = (E + T + L).upper()
    part = "ext" if t < len(E) else "target" if t < len(E) + len(T) else "lig"
    _pos, a, n, k, K_o, N_o, q = rec
    ref, alt = chr(M[t]), ALLELE_TEXT[a]
    if fields[17] == b"+":
        position, strand = int(fields[3]) + t, "+"
    else:
        position, strand = int(fields[4]) - t, "-"
        ref, alt = COMPLEMENT.get(ref, ref), COMPLEMENT.get(alt, alt)
    line = f"{sample}\t{fields[0].decode()}\t{fields[2].decode()}\t{position}\t{strand}\t{part}\t{ref}\t{alt}\t{n}\t{k}\t{k * MILLION // n}\t{K_o}\t{N_o}\t{q}\n"
    return ALLELE_TEXT.index(alt), line


def calls_file(tables: Sequence[np.ndarray], table_rows: Sequence[Sequence[bytes]], labels: Optional[Sequence[str]], p: Dict[str, int]):
    """(the -call file, its stderr line, candidates excluded by the band) from the count table of EVERY row of the session (with labels: the samples in file order,
    then undetermined), as pileup_ref.pileup or gapped_ref.pileup gives them.  Lines: rows first, then table order, then ascending t, then printed alt A C G T -."""
    mol = [(f[6] + f[13] + f[10]).upper() for f in table_rows]
    ref = b"".join(mol)
    owner = [(i, t) for i, m in enumerate(mol) for t in range(len(m))]
    n_sample = len(tables) - 1 if labels is not None else 1
    pool_ = pool(tables[:n_sample], p["bg_max_ppm"])
    out = [CALLS_HEADER]
    sums = {"calls": 0, "candidates": 0, "tested": 0, "too_deep": 0, "excluded": 0}
    for row, counts in enumerate(tables):
        sample = "*" if labels is None else labels[row] if row < len(labels) else "undetermined"
        totals, cands = call_cells(counts, pool_, ref, row < n_sample, p)
        for key in sums:
            sums[key] += totals[key]
        lines = []
        for rec in kept_calls(cands, p):
            i, t = owner[rec[0]]
            rank, line = call_line(sample, table_rows[i], t, rec)
            lines.append((rec[0], rank, line))
        out += [l for _, _, l in sorted(lines)]
    stderr = f"mipgen_count: calls {sums['calls']} candidates {sums['candidates']} tested {sums['tested']} too_deep {sums['too_deep']}\n"
    return "".join(out).encode(), stderr, sums["excluded"]
