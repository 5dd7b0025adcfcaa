"""The variant-calling model of DESIGN 4.14 restated by brute force (test oracle for mipgen_accel_call_tables, mipgen_accel_reads_consensus_call and
`mipgen_count -call`): plain loops over rows, positions and allele classes, and the binomial tail as an EXACT Python integer: the sum of C(n,i) A^i B^(n-i) over
ALL i = k..n with e = A / (A + B), over (A + B)^n.  No early stop, no log-gamma, no table; -10 log10 comes from math.log10 of the two big integers.  Test
infrastructure."""
import decimal
import math
from fractions import Fraction
from typing import Callable, Dict, List, Optional, Sequence, Tuple

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


# ---- the same score where the exact sum is out of reach: up to the depth cap --------------------------------------------------------------------------------
HP_FRACTION_BITS = 320               # of the fixed-point sum
HP_DIGITS = 80                       # of the decimal context the logarithms are taken in
HP_STIRLING_FROM = 1000              # ln m! from math.factorial below, from Stirling's series from here on
HP_STIRLING_TERMS = 8                # B_2j / (2j (2j-1) m^(2j-1)), j = 1..8


def _bernoulli(count: int) -> List[Fraction]:
    """B_0 .. B_count (B_1 = -1/2) from the recurrence sum_{j<=m} C(m+1, j) B_j = 0."""
    B = [Fraction(1)]
    for m in range(1, count + 1):
        B.append(-sum(math.comb(m + 1, j) * B[j] for j in range(m)) / (m + 1))
    return B


_HP_CTX = decimal.Context(prec=HP_DIGITS, rounding=decimal.ROUND_HALF_EVEN, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
_HP_BERNOULLI = _bernoulli(2 * HP_STIRLING_TERMS)
_HP_HALF_LN_2PI = None               # (set on first use: pi is not in the decimal module)
_hp_lnfact_cache: Dict[int, decimal.Decimal] = {}


def _hp_pi(ctx: decimal.Context) -> decimal.Decimal:
    """Machin: pi = 16 atan(1/5) - 4 atan(1/239), as scaled integers with 20 guard digits."""
    scale = 10 ** (HP_DIGITS + 20)

    def atan_inv(x: int) -> int:
        total, term, j = 0, scale // x, 0
        while term:
            total += term // (2 * j + 1) if j % 2 == 0 else -(term // (2 * j + 1))
            term //= x * x
            j += 1
        return total

    return ctx.divide(decimal.Decimal(16 * atan_inv(5) - 4 * atan_inv(239)), decimal.Decimal(scale))


def hp_lnfact(m: int) -> decimal.Decimal:
    """ln m! to about 1e-75 relative.  Below HP_STIRLING_FROM: the logarithm of the exact integer.  From there on Stirling's series (m + 1/2) ln m - m + ln(2 pi) / 2 +
    sum_{j=1..8} B_2j / (2j (2j-1) m^(2j-1)).  The series is asymptotic with terms of alternating sign, so what it leaves is smaller than the first dropped term,
    B_18 / (18 x 17 m^17) = 54.97 / 306 / m^17 < 1.8e-52 at m = 1,000 - far below the 1e-40 asked for."""
    global _HP_HALF_LN_2PI
    got = _hp_lnfact_cache.get(m)
    if got is not None:
        return got
    ctx, D = _HP_CTX, decimal.Decimal
    if m < HP_STIRLING_FROM:
        out = ctx.ln(D(math.factorial(m)))
    else:
        if _HP_HALF_LN_2PI is None:
            _HP_HALF_LN_2PI = ctx.divide(ctx.ln(ctx.multiply(D(2), _hp_pi(ctx))), D(2))
        series = Fraction(0)
        for j in range(1, HP_STIRLING_TERMS + 1):
            series += _HP_BERNOULLI[2 * j] / (2 * j * (2 * j - 1) * m ** (2 * j - 1))
        out = ctx.multiply(D(2 * m + 1) / 2, ctx.ln(D(m)))
        out = ctx.add(ctx.subtract(out, D(m)), _HP_HALF_LN_2PI)
        out = ctx.add(out, ctx.divide(D(series.numerator), D(series.denominator)))
    if len(_hp_lnfact_cache) < 4096:
        _hp_lnfact_cache[m] = out
    return out


def hp_phred(k: int, n: int, A: int, B: int) -> decimal.Decimal:
    """-10 log10 of P(X >= k), X binomial(n, A / B), for a k above expectation (k B > n A: the terms fall from k on) at any depth up to the cap, from the standard
    library alone: P = t_k S with S = sum_{i=k..n} t_i / t_k.
     - S in fixed point, Python integers with HP_FRACTION_BITS fractional bits: t <- t (n-i) a // ((i+1) b), a = A, b = B - A, from t = 1, run to i = n or until the
       fixed-point term is 0.  There is no relative early stop.  Truncation: every step floors once, which costs the term at most 1 unit in the last place, and the
       factor (n-i) a / ((i+1) b) is below 1, so it does not grow what the term carries: after j steps the term is at most j units low, the sum of m terms at most
       m^2 / 2 units.  When the fixed-point term reaches 0 after j steps the true term is below j + 1 units, and so is every later one, the terms falling: with
       n <= 2^20 all of that stays below 2^41 units = 2^-279 of an S >= 1.
     - ln t_k = ln n! - ln k! - ln (n-k)! + k ln(a / B) + (n-k) ln(b / B) in `decimal` at HP_DIGITS digits (hp_lnfact); the magnitudes that meet are below 1e8, so
       the result carries about 1e-70.  No math.comb: at k about n / 2 and n = 2^20 it takes tens of seconds.
    Returns a Decimal."""
    a, b = A, B - A
    assert 0 < a < B and 0 <= k <= n and k * B > n * a
    one = 1 << HP_FRACTION_BITS
    t = total = one
    for i in range(k, n):
        t = t * ((n - i) * a) // ((i + 1) * b)
        if t == 0:
            break
        total += t
    ctx, D = _HP_CTX, decimal.Decimal
    ln_B = ctx.ln(D(B))
    ln_tk = ctx.subtract(ctx.subtract(hp_lnfact(n), hp_lnfact(k)), hp_lnfact(n - k))
    ln_tk = ctx.add(ln_tk, ctx.multiply(D(k), ctx.subtract(ctx.ln(D(a)), ln_B)))
    ln_tk = ctx.add(ln_tk, ctx.multiply(D(n - k), ctx.subtract(ctx.ln(D(b)), ln_B)))
    ln_S = ctx.subtract(ctx.ln(D(total)), ctx.multiply(D(HP_FRACTION_BITS), ctx.ln(D(2))))
    return ctx.divide(ctx.multiply(D(-10), ctx.add(ln_tk, ln_S)), ctx.ln(D(10)))


def hp_text(score: decimal.Decimal) -> str:
    """The decimal string of a high-precision score as the fixtures hold it: 30 places."""
    return str(score.quantize(decimal.Decimal(1).scaleb(-30), rounding=decimal.ROUND_HALF_EVEN, context=_HP_CTX))


def near_integer(phred) -> bool:
    """Within DELTA of an integer at or below the cap - the floor could go either way - and so within DELTA of the cap itself."""
    if phred > Q_CAP + DELTA:
        return False
    return abs(phred - round(phred)) <= DELTA


def q_of(phred: float) -> int:
    return min(Q_CAP, max(0, math.floor(phred)))


def call_cells(counts: np.ndarray, pool_: np.ndarray, ref: bytes, own_row_is_sample: bool, p: Dict[str, int], filters_only: bool = False,
               score: Callable[[int, int, int, int], object] = exact_phred):
    """(totals dict, candidates): every candidate as a dict of the record's fields plus `phred` (exact, before the floor; None with filters_only or above the depth
    the exact sum is asked for) and `excluded` (near_integer).  score: exact_phred, or hp_phred for tables deeper than the exact sum can go.  Ascending (pos, allele).  totals["calls"] counts candidates with q >= min_q that are not excluded;
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
                rec["phred"] = score(k, n, K_o + p["a0"], N_o + p["n0"])
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
