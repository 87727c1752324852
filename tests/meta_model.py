"""Referees that need neither the CPU oracle nor the library: exact invariances of the chain partitioning problem, the objectives
straight from their definitions, and optimality certificates computed on the host in O(nnz).  Pure numpy; shares no code with
oracle/, with the layer functions of tests/brute.py or with the kernels.

  transforms of a pattern   relabel_rows, mirror_columns, reverse_rows, shift_rows, mirror_both
  transforms of a model     scaled, shifted
  definition-level values   pins / nets / selfnets / span of a column range by np.unique, part_cost, total, bottleneck
  pair_optimal              every interior boundary is the best place between its two neighbours (necessary for a total-cost optimum)
  greedy_parts              the fewest parts of cost <= c; for a cost that grows with the range the bottleneck c of a K-split is
                            optimal iff greedy_parts(c) <= K < greedy_parts(c - step)
  bottleneck_optimum        bisection on c over greedy_parts

Split vectors are 1-based as the library returns them (part k = columns spl[k] : spl[k + 1] - 1); everything inside works on 0-based
boundary positions.  The models are told apart by their class names and read through their attributes: AffineWorkModel,
AffineConnectivityModel, AffineHyperedgeCutModel, AffineEnvelopeModel; the three symmetric models on a square pattern (dianet: the rows
of a column range united with its own indices, selfpin: the entries of its diagonal block); and -- with a partition Pi of the rows, a
MapPartition or a SplitPartition -- the primary connectivity and primary edge-cut models and the secondary connectivity model, whose
part number k (1-based) enters the counts.  No per-part alpha.

What referees what: part_cost is the definition by np.unique / set operations; left_costs / right_costs are its window forms, checked
against part_cost and against the dense tables of brute.py, sym_model.py and plaid_total_model.py at small n by
tests/test_meta_model.py; at n = 4 099 and 70 001 tests/test_gpu_metamorphic.py holds the library's split vectors to the invariances
and to pair_slack == 0 computed here alone."""
import numpy as np

INFEASIBLE = 1 << 62


# ---------------------------------------------------------------- transforms of a pattern
def _entries(A):
    """0-based (cols, rows) of the stored entries"""
    pos = np.asarray(A.colptr, dtype=np.int64) - 1
    return np.repeat(np.arange(A.n, dtype=np.int64), np.diff(pos)), np.asarray(A.rowval, dtype=np.int64) - 1


def _pattern(like, m, n, cols, rows):
    """a pattern of like's class from 0-based entries, rows ascending inside each column"""
    key = np.sort(cols * np.int64(m + 1) + rows)
    c, r = key // (m + 1), key % (m + 1)
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64)
    return type(like)(m, n, colptr, r + 1)


def relabel_rows(A, rng, extra=0, return_map=False):
    """A[sigma, :] for a random injection sigma of the m rows into m + extra rows (the extras stay empty and change the heights of the
    counting structures).  return_map: also sigma, 0-based, new row = sigma[old row]"""
    cols, rows = _entries(A)
    sigma = rng.permutation(A.m + extra)[:A.m].astype(np.int64)
    B = _pattern(A, A.m + extra, A.n, cols, sigma[rows])
    return (B, sigma) if return_map else B


def mirror_columns(A):
    """column j -> n + 1 - j"""
    cols, rows = _entries(A)
    return _pattern(A, A.m, A.n, A.n - 1 - cols, rows)


def reverse_rows(A):
    """row i -> m + 1 - i"""
    cols, rows = _entries(A)
    return _pattern(A, A.m, A.n, cols, A.m - 1 - rows)


def shift_rows(A, d):
    """d empty rows in front"""
    cols, rows = _entries(A)
    return _pattern(A, A.m + d, A.n, cols, rows + d)


def mirror_both(A):
    """row i -> n + 1 - i and column j -> n + 1 - j of a square pattern: dianet, selfpin and net of a range become those of its mirror"""
    cols, rows = _entries(A)
    return _pattern(A, A.m, A.n, A.n - 1 - cols, A.m - 1 - rows)


def mirror_split(spl, n):
    """the split vector of the mirrored parts on mirror_columns(A)"""
    return (n + 2 - np.asarray(spl, dtype=np.int64))[::-1].copy()


# ---------------------------------------------------------------- transforms of a model
def scaled(mdl, c):
    """every parameter times the integer c"""
    return type(mdl)(*[p * c for p in mdl._params()])


def shifted(mdl, a):
    """alpha + a"""
    p = mdl._params()
    return type(mdl)(p[0] + a, *p[1:])


# ---------------------------------------------------------------- values from the definition
def _kind(mdl):
    return {"AffineWorkModel": "work", "AffineConnectivityModel": "conn", "AffineHyperedgeCutModel": "hcut", "AffineEnvelopeModel": "env",
            "AffinePrimaryConnectivityModel": "prim", "AffinePrimaryEdgeCutModel": "pcut", "AffineSecondaryConnectivityModel": "sec",
            "AffineSymmetricConnectivityModel": "symc", "AffineMonotonizedSymmetricConnectivityModel": "msym",
            "AffineSymmetricEdgeCutModel": "scut"}[type(mdl).__name__]


def row_owner(Pi, m):
    """the 1-based part of every row under a MapPartition or a SplitPartition"""
    if hasattr(Pi, "asg"):
        return np.asarray(Pi.asg, dtype=np.int64)
    return np.searchsorted(np.asarray(Pi.spl, dtype=np.int64), np.arange(1, m + 1), side="right").astype(np.int64)


def _range_rows(A, j, jp):
    return np.asarray(A.rowval)[A.colptr[j - 1] - 1:A.colptr[jp - 1] - 1]


def pins(A, j, jp):
    return int(A.colptr[jp - 1] - A.colptr[j - 1])


def nets(A, j, jp):
    """distinct rows of the columns j : j' - 1"""
    return int(np.unique(_range_rows(A, j, jp)).size)


def selfnets(A, j, jp):
    """rows whose whole support lies in the columns j : j' - 1"""
    rv = np.asarray(A.rowval)
    outside = np.concatenate([rv[:A.colptr[j - 1] - 1], rv[A.colptr[jp - 1] - 1:]])
    return int(np.setdiff1d(np.unique(_range_rows(A, j, jp)), np.unique(outside)).size)


def span(A, j, jp):
    """greatest minus least row of the columns j : j' - 1, 0 without entries"""
    r = _range_rows(A, j, jp)
    return int(r.max() - r.min()) if r.size else 0


def dianets(A, j, jp):
    """the rows of the columns j : j' - 1 united with j : j' - 1 themselves"""
    return int(np.union1d(_range_rows(A, j, jp), np.arange(j, jp)).size)


def selfpins(A, j, jp):
    """the entries of the block A[j : j' - 1, j : j' - 1]"""
    r = _range_rows(A, j, jp)
    return int(((r >= j) & (r < jp)).sum())


def overpins(A, j, jp, delta):
    deg = np.diff(np.asarray(A.colptr, dtype=np.int64))[j - 1:jp - 1]
    return int(np.maximum(deg - int(delta), 0).sum())


def split_selfnets(A, spl):
    """selfnets of every part of a split at once: the rows whose first and last column lie in one part, counted per part (the
    definition of selfnets(), one O(nnz) pass per part, is too slow for the thousands of parts a narrow chunker makes)"""
    ix = index(A)
    spl = np.asarray(spl, dtype=np.int64)
    hit = ix.last >= 0
    first = np.searchsorted(spl, ix.first[hit] + 1, side="right") - 1       # (side right: of equal boundaries the last, the non-empty part)
    last = np.searchsorted(spl, ix.last[hit] + 1, side="right") - 1
    return np.bincount(first[first == last], minlength=spl.size - 1)


def part_cost(A, mdl, j, jp, k=None, Pi=None, n_self=None):
    """f(j, j', k) from the definition, in Python numbers (n_self: the part's self nets where split_selfnets has counted them)"""
    kind = _kind(mdl)
    if kind == "sec":                                              # the rows, pins and columns of part k; local: its columns inside j : j' - 1
        own = row_owner(Pi, A.m)
        cols, rows = _entries(A)
        mine = np.unique(cols[own[rows] == k]) + 1
        inside = int(((mine >= j) & (mine < jp)).sum())
        return (mdl.alpha + int((own == k).sum()) * mdl.beta_vertex + int((own[rows] == k).sum()) * mdl.beta_pin
                + inside * mdl.beta_local_net + (int(mine.size) - inside) * mdl.beta_remote_net)
    v = mdl.alpha + (jp - j) * mdl.beta_vertex
    if kind == "msym":
        return v + overpins(A, j, jp, mdl.delta_pins) * mdl.beta_over_pin + dianets(A, j, jp) * mdl.beta_dia_net
    if kind == "scut":
        return v + selfpins(A, j, jp) * mdl.beta_self_pin + (pins(A, j, jp) - selfpins(A, j, jp)) * mdl.beta_cut_pin
    if kind != "pcut":
        v = v + pins(A, j, jp) * mdl.beta_pin
    if kind == "symc":
        rem = dianets(A, j, jp) - (jp - j)
        return v + (nets(A, j, jp) - rem) * mdl.beta_local_net + rem * mdl.beta_remote_net
    if kind == "conn":
        v = v + nets(A, j, jp) * mdl.beta_net
    elif kind == "hcut":
        s = selfnets(A, j, jp) if n_self is None else int(n_self)
        v = v + s * mdl.beta_self_net + (nets(A, j, jp) - s) * mdl.beta_cut_net
    elif kind == "env":
        v = v + span(A, j, jp) * mdl.beta_net
    elif kind == "prim":
        own = row_owner(Pi, A.m)[np.unique(_range_rows(A, j, jp)) - 1] == k
        v = v + int(own.sum()) * mdl.beta_local_net + int((~own).sum()) * mdl.beta_remote_net
    elif kind == "pcut":
        own = row_owner(Pi, A.m)[_range_rows(A, j, jp) - 1] == k
        v = v + int(own.sum()) * mdl.beta_self_pin + int((~own).sum()) * mdl.beta_cut_pin
    return v


def part_costs(A, mdl, spl, Pi=None):
    own = split_selfnets(A, spl) if _kind(mdl) == "hcut" else None
    spl = [int(s) for s in np.asarray(spl)]
    return [part_cost(A, mdl, spl[k], spl[k + 1], k + 1, Pi, None if own is None else own[k]) for k in range(len(spl) - 1)]


def total(A, mdl, spl, Pi=None):
    return sum(part_costs(A, mdl, spl, Pi))


def bottleneck(A, mdl, spl, Pi=None):
    return max(part_costs(A, mdl, spl, Pi))


def structure_ok(A, spl, w=None, budget=None):
    """spl[0] = 1, spl[-1] = n + 1, sorted, widths and pins within their limits"""
    spl = np.asarray(spl, dtype=np.int64)
    ok = spl[0] == 1 and spl[-1] == A.n + 1 and bool(np.all(np.diff(spl) >= 0))
    if ok and w is not None:
        ok = bool(np.all(np.diff(spl) <= w))
    if ok and budget is not None:
        pos = np.asarray(A.colptr, dtype=np.int64)
        ok = bool(np.all(pos[spl[1:] - 1] - pos[spl[:-1] - 1] <= budget))
    return bool(ok)


# ---------------------------------------------------------------- one sweep per window
class Index:
    """per entry the previous and the next column that holds its row, per row its first and last column, per column its least and
    greatest row: one stable sort of the entries by row"""

    def __init__(self, A):
        self.A, self.n, self.m = A, A.n, A.m
        self.pos = np.asarray(A.colptr, dtype=np.int64) - 1
        self.cols, self.rows = _entries(A)
        nnz, n, m = self.rows.size, A.n, A.m
        order = np.argsort(self.rows, kind="stable")              # by (row, column): the columns ascend in storage order
        rs, cs = self.rows[order], self.cols[order]
        same = rs[1:] == rs[:-1]
        self.prev = np.full(nnz, -1, dtype=np.int64); self.prev[order[1:][same]] = cs[:-1][same]
        self.next = np.full(nnz, n, dtype=np.int64); self.next[order[:-1][same]] = cs[1:][same]
        self.first = np.full(m, n, dtype=np.int64); self.last = np.full(m, -1, dtype=np.int64)
        head = np.concatenate([[True], ~same]) if nnz else np.zeros(0, bool)
        tail = np.concatenate([~same, [True]]) if nnz else np.zeros(0, bool)
        self.first[rs[head]] = cs[head]; self.last[rs[tail]] = cs[tail]
        self.collo = np.full(n, m, dtype=np.int64); self.colhi = np.full(n, -1, dtype=np.int64)      # (m, -1): a column without entries
        full = np.diff(self.pos) > 0
        self.collo[full] = self.rows[self.pos[:-1][full]]; self.colhi[full] = self.rows[self.pos[1:][full] - 1]


_INDEX = {}


def index(A):
    if id(A) not in _INDEX:
        if len(_INDEX) > 64:
            _INDEX.clear()
        _INDEX[id(A)] = Index(A)                                   # (the Index keeps A alive, so the id stays its own)
    return _INDEX[id(A)]


def _below(x, lo, hi):
    """out[t - lo] = #{x < t} for t = lo .. hi, for values lo <= x < hi"""
    return np.concatenate([[0], np.cumsum(np.bincount(x - lo, minlength=hi - lo))]).astype(np.int64)


def _affine(ix, mdl, nv, npins, terms):
    dt = np.int64 if mdl.dtype == 0 else np.float64
    v = dt(mdl.alpha) + nv.astype(dt) * dt(mdl.beta_vertex)
    if _kind(mdl) not in ("pcut", "msym", "scut", "sec"):
        v = v + npins.astype(dt) * dt(mdl.beta_pin)
    for count, beta in terms:
        v = v + count.astype(dt) * dt(beta)
    return v


def _sym_terms(ix, mdl, a, b, t, lo, hi, entered, diag_key, count):
    """the terms of a symmetric model over the windows [lo, hi) inside [a, b).  entered: the one entry per row that brings the row in
    (its first at or after a / its last before b), diag_key: min or max, the rule that joins a row's own diagonal position to that entry,
    count: keys -> how many count at every t"""
    pos, kind = ix.pos, _kind(mdl)
    sl = slice(pos[a], pos[b])
    i, c = ix.rows[sl], ix.cols[sl]
    if kind == "scut":
        ok = (i >= a) & (i < b)                                    # an entry lies in the block once both its indices do
        own = count(diag_key(i[ok], c[ok]))
        return [(own, mdl.beta_self_pin), (pos[hi] - pos[lo] - own, mdl.beta_cut_pin)]
    key = np.arange(a, b, dtype=np.int64)                          # the rows a .. b - 1 count from their own position on ...
    ie, ce = i[entered], c[entered]
    inside = (ie >= a) & (ie < b)
    key[ie[inside] - a] = diag_key(ie[inside], ce[inside])         # ... or from the entry that brings them in, whichever comes first
    dia = count(np.concatenate([key, ce[~inside]]))
    if kind == "msym":
        over = np.concatenate([[0], np.cumsum(np.maximum(np.diff(pos) - int(mdl.delta_pins), 0))])
        return [(over[hi] - over[lo], mdl.beta_over_pin), (dia, mdl.beta_dia_net)]
    rem = dia - (hi - lo)
    return [(count(ce) - rem, mdl.beta_local_net), (rem, mdl.beta_remote_net)]


def _sec_parts(ix, mdl, k, Pi):
    """the secondary model's part k: the flag of every column that holds one of its rows, and its constant terms"""
    own = row_owner(Pi, ix.m)
    mine = own[ix.rows] == k
    has = np.bincount(ix.cols[mine], minlength=ix.n) > 0
    dt = np.int64 if mdl.dtype == 0 else np.float64
    const = dt(mdl.alpha) + dt(int((own == k).sum())) * dt(mdl.beta_vertex) + dt(int(mine.sum())) * dt(mdl.beta_pin)
    return has, int(has.sum()), const, dt


def left_costs(ix, mdl, a, b, k=None, Pi=None):
    """f of the columns [a, t) for t = a .. b (0-based positions)"""
    pos, kind = ix.pos, _kind(mdl)
    if kind in ("symc", "msym", "scut"):
        t = np.arange(a, b + 1, dtype=np.int64)
        terms = _sym_terms(ix, mdl, a, b, t, a, t, ix.prev[pos[a]:pos[b]] < a, np.maximum if kind == "scut" else np.minimum, lambda x: _below(x, a, b))
        return _affine(ix, mdl, t - a, pos[t] - pos[a], terms)
    if kind == "sec":
        has, d, const, dt = _sec_parts(ix, mdl, k, Pi)
        loc = np.concatenate([[0], np.cumsum(has[a:b])]).astype(np.int64)
        return const + loc.astype(dt) * dt(mdl.beta_local_net) + (d - loc).astype(dt) * dt(mdl.beta_remote_net)
    sl = slice(pos[a], pos[b])
    t = np.arange(a, b + 1, dtype=np.int64)
    c = ix.cols[sl]
    terms = []
    if kind in ("conn", "hcut", "prim"):
        new = ix.prev[sl] < a                                      # the first entry of its row at or after column a
        net = _below(c[new], a, b)
    if kind == "conn":
        terms = [(net, mdl.beta_net)]
    elif kind == "hcut":
        whole = ix.last[ix.rows[sl][ix.prev[sl] < 0]]              # rows that begin inside, by their last column
        own = _below(whole[whole < b], a, b)                       # #{last < t}
        terms = [(own, mdl.beta_self_net), (net - own, mdl.beta_cut_net)]
    elif kind == "env":
        lo = np.concatenate([[ix.m], np.minimum.accumulate(ix.collo[a:b])])
        hi = np.concatenate([[-1], np.maximum.accumulate(ix.colhi[a:b])])
        terms = [(np.maximum(hi - lo, 0), mdl.beta_net)]
    elif kind == "prim":
        loc = _below(c[new & (row_owner(Pi, ix.m)[ix.rows[sl]] == k)], a, b)
        terms = [(loc, mdl.beta_local_net), (net - loc, mdl.beta_remote_net)]
    elif kind == "pcut":
        own = _below(c[row_owner(Pi, ix.m)[ix.rows[sl]] == k], a, b)
        terms = [(own, mdl.beta_self_pin), (pos[t] - pos[a] - own, mdl.beta_cut_pin)]
    return _affine(ix, mdl, t - a, pos[t] - pos[a], terms)


def right_costs(ix, mdl, a, b, k=None, Pi=None):
    """f of the columns [t, b) for t = a .. b"""
    pos, kind = ix.pos, _kind(mdl)
    if kind in ("symc", "msym", "scut"):
        t = np.arange(a, b + 1, dtype=np.int64)
        at_least = lambda x: x.size - _below(x, a, b)
        terms = _sym_terms(ix, mdl, a, b, t, t, b, ix.next[pos[a]:pos[b]] >= b, np.minimum if kind == "scut" else np.maximum, at_least)
        return _affine(ix, mdl, b - t, pos[b] - pos[t], terms)
    if kind == "sec":
        has, d, const, dt = _sec_parts(ix, mdl, k, Pi)
        loc = np.concatenate([np.cumsum(has[a:b][::-1])[::-1], [0]]).astype(np.int64)
        return const + loc.astype(dt) * dt(mdl.beta_local_net) + (d - loc).astype(dt) * dt(mdl.beta_remote_net)
    sl = slice(pos[a], pos[b])
    t = np.arange(a, b + 1, dtype=np.int64)
    c = ix.cols[sl]
    at_least = lambda x: x.size - _below(x, a, b)                  # #{x >= t}
    terms = []
    if kind in ("conn", "hcut", "prim"):
        end = ix.next[sl] >= b                                     # the last entry of its row before column b
        net = at_least(c[end])
    if kind == "conn":
        terms = [(net, mdl.beta_net)]
    elif kind == "hcut":
        whole = ix.first[ix.rows[sl][ix.next[sl] >= ix.n]]         # rows that end inside, by their first column
        whole = whole[whole >= a]
        own = at_least(whole)
        terms = [(own, mdl.beta_self_net), (net - own, mdl.beta_cut_net)]
    elif kind == "env":
        lo = np.concatenate([np.minimum.accumulate(ix.collo[a:b][::-1])[::-1], [ix.m]])
        hi = np.concatenate([np.maximum.accumulate(ix.colhi[a:b][::-1])[::-1], [-1]])
        terms = [(np.maximum(hi - lo, 0), mdl.beta_net)]
    elif kind == "prim":
        loc = at_least(c[end & (row_owner(Pi, ix.m)[ix.rows[sl]] == k)])
        terms = [(loc, mdl.beta_local_net), (net - loc, mdl.beta_remote_net)]
    elif kind == "pcut":
        own = at_least(c[row_owner(Pi, ix.m)[ix.rows[sl]] == k])
        terms = [(own, mdl.beta_self_pin), (pos[b] - pos[t] - own, mdl.beta_cut_pin)]
    return _affine(ix, mdl, b - t, pos[b] - pos[t], terms)


def pair_slack(A, mdl, spl, w=None, budget=None, Pi=None):
    """per pair of neighbouring parts [s_k, s_k+2): f(s_k, s_k+1) + f(s_k+1, s_k+2) minus the least such sum over the feasible t (both
    widths <= w, both pin counts <= budget).  The boundary itself must be feasible."""
    ix = index(A)
    s = np.asarray(spl, dtype=np.int64) - 1
    out = []
    for k in range(len(s) - 2):
        a, mid, b = int(s[k]), int(s[k + 1]), int(s[k + 2])
        v = left_costs(ix, mdl, a, b, k + 1, Pi) + right_costs(ix, mdl, a, b, k + 2, Pi)
        t = np.arange(a, b + 1, dtype=np.int64)
        ok = np.ones(t.size, dtype=bool)
        if w is not None:
            ok &= (t - a <= w) & (b - t <= w)
        if budget is not None:
            ok &= (ix.pos[t] - ix.pos[a] <= budget) & (ix.pos[b] - ix.pos[t] <= budget)
        assert ok[mid - a], "the split itself breaks its limits"
        out.append(v[mid - a] - v[ok].min())
    return out


def pair_optimal(A, mdl, spl, w=None, budget=None, Pi=None):
    return all(x == 0 for x in pair_slack(A, mdl, spl, w, budget, Pi))


# ---------------------------------------------------------------- the bottleneck certificate
def grows(mdl):
    """the cost of a range never falls when the range grows"""
    kind = _kind(mdl)
    if kind == "hcut":
        return mdl.beta_vertex >= 0 and mdl.beta_pin >= 0 and mdl.beta_self_net >= mdl.beta_cut_net >= 0
    return kind in ("work", "conn", "env") and all(p >= 0 for p in mdl._params()[1:])


def greedy_parts(A, mdl, c, w=None, budget=None, limit=None):
    """the fewest parts with every part's cost <= c (and width <= w, pins <= budget): each part takes columns while it fits.  Exact
    for a cost that grows().  INFEASIBLE if some column fits no part; limit: stop counting past that many parts."""
    assert grows(mdl)
    ix = index(A)
    n, pos = ix.n, ix.pos
    if mdl.alpha > c:
        return INFEASIBLE
    a, parts, guess = 0, 0, 64
    while a < n:
        cap = n if w is None else min(n, a + int(w))
        if budget is not None:
            cap = min(cap, int(np.searchsorted(pos, pos[a] + budget, side="right")) - 1)
        while True:
            hi = min(cap, a + guess)
            fit = int(np.searchsorted(left_costs(ix, mdl, a, hi), c, side="right")) - 1 if hi > a else 0
            if fit < hi - a or hi == cap:
                break
            guess *= 2
        if fit < 1:
            return INFEASIBLE
        a, parts, guess = a + fit, parts + 1, max(64, 2 * fit)
        if limit is not None and parts > limit:
            return parts
    return max(parts, 1)


def certified(A, mdl, K, c, w=None, budget=None, step=1):
    """c is the least bottleneck of a K-split: K parts of cost <= c exist, K parts of cost <= c - step do not (step: the grid all
    costs of the model lie on)"""
    return greedy_parts(A, mdl, c, w, budget, limit=K) <= K < greedy_parts(A, mdl, c - step, w, budget, limit=K)


def bottleneck_optimum(A, mdl, K, w=None, budget=None, step=1):
    """the least c on the grid of step with greedy_parts(c) <= K; None if no K-split keeps the limits"""
    ix = index(A)
    hi = int(np.ceil(float(left_costs(ix, mdl, 0, ix.n)[-1]) / step))
    if greedy_parts(A, mdl, hi * step, w, budget, limit=K) > K:
        return None
    lo = int(np.floor(mdl.alpha / step)) - 1                                   # (below alpha nothing fits)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if greedy_parts(A, mdl, mid * step, w, budget, limit=K) <= K:
            hi = mid
        else:
            lo = mid
    return hi * step


def most_parts(A, mdl, c, limit=None):
    """the most parts with every part's cost >= c > alpha, for a cost that grows(): each part closes as soon as it reaches c and the last
    one takes the rest.  limit: stop counting at that many parts."""
    assert grows(mdl) and c > mdl.alpha
    ix = index(A)
    n, a, parts, guess = ix.n, 0, 0, 64
    while a < n and (limit is None or parts < limit):
        while True:
            hi = min(n, a + guess)
            need = int(np.searchsorted(left_costs(ix, mdl, a, hi), c, side="left"))
            if need <= hi - a or hi == n:
                break
            guess *= 2
        if need > hi - a:
            break
        a, parts, guess = a + need, parts + 1, max(64, 2 * need)
    return parts


def maxmin_optimum(A, mdl, K, step=1):
    """the greatest c on the grid of step such that K parts of cost >= c each exist (the bottleneck of the decreasing cost c0 - f is c0
    minus this); alpha itself if there is none"""
    ix = index(A)
    lo = int(np.floor(mdl.alpha / step))
    hi = int(np.ceil(float(left_costs(ix, mdl, 0, ix.n)[-1]) / step)) + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if most_parts(A, mdl, mid * step, limit=K) >= K:
            lo = mid
        else:
            hi = mid
    return lo * step
