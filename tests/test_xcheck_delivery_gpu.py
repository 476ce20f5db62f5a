"""GPU: every delivery of the cross-check + ratio test of ONE small pair, side by side.  The other files cover one or two
deliveries each; none covers the choice between the direct (page-locked) and the staged compaction.  Expected values come
from the oracle alone: cross-check, float64 ratio against oracle.self_dist, ratio < tau in ascending query index (as
test_gather_gpu.py derives them); every delivery must equal that list, cut at its capacity, bit for bit.

Shape: 700 x 900 rows -- three 256-row compaction blocks (the last one partial), nq no multiple of 64, both banks padded;
two splits are forced through the "nsplit" option.  Pairs: planted SIFT-like rows (integer route), kat.far_banks (every
distance in the float32-root tie range: the tie list and its repair run behind every delivery), a non-integer float32 pair,
and -- for the plain cross-check -- 32-byte binary rows."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hamming_ref
import kat
import oracle
from fastmatch_amd import sharding, synth

pytestmark = pytest.mark.gpu

NQ, NT = 700, 900
SENT = -7
# chosen on the CPU so that between 100 and 600 of the 700 rows are accepted (asserted where they are used)
TAU = {"planted": 0.7, "far": 2551.0, "f32": 0.7}


def _f32_pair(nq, nt, seed):
    """Non-integer float32 rows with planted near pairs (float32 route; the oracle's order-1 chain is its reference)."""
    rng = np.random.default_rng(seed)
    Q, T, _ = synth.planted_pair(nq, nt, seed)
    jit = lambda a: (a.astype(np.float32) + rng.uniform(-0.5, 0.5, a.shape).astype(np.float32)).astype(np.float32)
    return jit(Q), jit(T)


@functools.lru_cache(maxsize=None)
def _pair(name, nq=NQ, nt=NT):
    """(Q, T, the oracle's self distances of Q, the oracle's cross-check (tidx, dist))"""
    if name == "planted":
        Q, T, _ = synth.planted_pair(nq, nt, seed=nq + nt)
    elif name == "far":
        Q, T = kat.far_banks(nq, nt, np.random.default_rng(5))
    else:
        Q, T = _f32_pair(nq, nt, seed=17)
    order = 1 if name == "f32" else 0
    return Q, T, oracle.self_dist(Q, order=order), oracle.bf_xcheck1(Q, T, order=order)


@functools.lru_cache(maxsize=None)
def _expect(name, nq=NQ, nt=NT, tau=None):
    """(per query row: tidx, dist, ratio, pass; the accepted rows in ascending query index: qidx, tidx, dist, ratio)"""
    _, _, sd, (otidx, odist) = _pair(name, nq, nt)
    m = np.nonzero(otidx >= 0)[0]
    oratio, opass = oracle.ratio_filter(odist[m], sd, TAU[name] if tau is None else tau, qrows=m.astype(np.int32))
    ratio = np.full(nq, np.nan)
    ratio[m] = oratio
    passed = np.zeros(nq, bool)
    passed[m] = opass
    keep = m[opass]
    return (otidx, odist, ratio, passed), (keep.astype(np.int32), otidx[keep], odist[keep], oratio[opass])


@pytest.fixture(scope="module")
def c():
    import fastmatch_amd
    ctx = fastmatch_amd.Context(0)
    ctx.set_option("nsplit", 2)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def banks(c):
    made = {}

    def get(name, nq=NQ, nt=NT):
        if (name, nq, nt) not in made:
            Q, T, sd, _ = _pair(name, nq, nt)
            qb, tb = c.bank(Q), c.bank(T)
            qb.set_selfdist(sd)
            made[(name, nq, nt)] = (qb, tb)
        return made[(name, nq, nt)]
    return get


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host_out(c, cap, pinned):
    mk = c.pinned_empty if pinned else (lambda n, dt: np.empty(n, dt))
    out = tuple(mk(cap, dt) for dt in (np.int32, np.int32, np.float32, np.float64))
    for a in out:
        a[...] = SENT
    return out


def _check_host(out, count, acc, cap, what):
    """The first min(full, cap) rows equal the oracle's list, the rest keeps the sentinel, the count is the full number."""
    m = min(len(acc[0]), cap)
    if count is not None:
        assert int(count) == len(acc[0]), (what, int(count), len(acc[0]))
    for got, want in zip(out, acc):
        assert _same(got[:m], want[:m]), what
        assert (got[m:] == SENT).all(), what


def _dev_buffers(c, cap, n=1):
    import torch
    dev = torch.device("cuda", c.device)
    return (torch.full((n, max(cap, 1), 3), SENT, dtype=torch.int32, device=dev), torch.full((n,), SENT, dtype=torch.int64, device=dev))


def _check_dev(rows, count, acc, cap, what):
    """Device rows: min(full, cap) packed rows, the sentinel behind them, the device word = the rows that are there."""
    m = min(len(acc[0]), cap)
    assert int(count) == m, (what, int(count), m)
    got = rows.cpu().numpy()
    assert _same(got[:m], sharding.pack_matches(acc[0][:m], acc[1][:m], acc[2][:m])), what
    assert (got[m:] == SENT).all(), what


def _all_deliveries(c, qb, tb, tau, full, acc, f32):
    """Every delivery the pair's kind admits; `full` / `acc`: what they must deliver (None: checked by the caller's own rule)."""
    import torch
    nq, n_acc = qb.n, len(acc[0])
    # match_ratio: one row per query, pageable and page-locked
    for pinned in ((False, True) if nq else (False,)):
        out = None
        if pinned:
            out = (c.pinned_empty(nq, np.int32), c.pinned_empty(nq, np.float32), c.pinned_empty(nq, np.float64), c.pinned_empty(nq, np.uint8))
        tidx, dist, ratio, passed, npass = c.match_ratio(qb, tb, tau, out=out)
        what = "match_ratio pinned=%s" % pinned
        assert npass == n_acc, what
        if nq:
            assert _same(tidx, full[0]) and _same(dist, full[1]) and _same(passed.astype(bool), full[3]), what
            assert _same(ratio[full[0] >= 0], full[2][full[0] >= 0]) and np.isnan(ratio[full[0] < 0]).all(), what
    # match_accepted: default outputs, then (pageable | page-locked) x (capacity 50 | nq + 50)
    got = c.match_accepted(qb, tb, tau)
    assert len(got[0]) == n_acc and all(_same(g, w) for g, w in zip(got, acc)), "match_accepted default"
    for pinned, cap in ((False, 50), (True, 50), (True, nq + 50)):        # (page-locked: the direct path, then the staged one)
        out = _host_out(c, cap, pinned)
        got = c.match_accepted(qb, tb, tau, out=out)
        assert len(got[0]) == min(n_acc, cap)
        _check_host(out, None, acc, cap, "match_accepted pinned=%s cap=%d" % (pinned, cap))
    # device rows, synchronous
    for cap in (50, max(nq, 1)):
        rows, count = _dev_buffers(c, cap)
        n = c.match_accepted_dev(qb, tb, tau, rows.data_ptr(), count.data_ptr(), cap)
        assert n == n_acc, "match_accepted_dev cap=%d" % cap
        _check_dev(rows[0], count[0], acc, cap, "match_accepted_dev cap=%d" % cap)
    if f32:
        return
    # the enqueue-only forms
    for cap in (50, max(nq, 1)):
        out, cnt = _host_out(c, cap, True), c.pinned_empty(1, np.int64)
        cnt[0] = SENT
        c.match_accepted_async(qb, tb, tau, out, cnt)
        c.sync()
        _check_host(out, cnt[0], acc, cap, "match_accepted_async cap=%d" % cap)
        for with_word in (False, True):
            rows, count = _dev_buffers(c, cap)
            torch.cuda.synchronize()
            hc = c.pinned_empty(1, np.int64) if with_word else None
            if with_word:
                hc[0] = SENT
            c.match_accepted_dev_async(qb, tb, tau, rows.data_ptr(), count.data_ptr(), cap, h_count=hc)
            c.sync()
            what = "match_accepted_dev_async cap=%d word=%s" % (cap, with_word)
            _check_dev(rows[0], count[0], acc, cap, what)
            if with_word:
                assert int(hc[0]) == n_acc, what
    # a batch of one pair: the single-pair branch
    out, cnt = _host_out(c, 50, True), c.pinned_empty(1, np.int64)
    cnt[0] = SENT
    c.match_accepted_batch([(qb, tb)], tau, [out], [cnt])
    c.sync()
    _check_host(out, cnt[0], acc, 50, "match_accepted_batch, one pair")
    rows, counts = _dev_buffers(c, 50)
    torch.cuda.synchronize()
    hcs = c.pinned_empty(1, np.int64)
    hcs[0] = SENT
    c.match_accepted_dev_batch([(qb, tb)], tau, rows.data_ptr(), counts.data_ptr(), 50, h_counts=hcs)
    c.sync()
    _check_dev(rows[0], counts[0], acc, 50, "match_accepted_dev_batch, one pair")
    assert int(hcs[0]) == n_acc


@pytest.mark.parametrize("name", ["planted", "far", "f32"])
def test_every_delivery_equals_the_oracle_list(c, banks, name):
    full, acc = _expect(name)
    assert 100 <= len(acc[0]) <= 600
    qb, tb = banks(name)
    _all_deliveries(c, qb, tb, TAU[name], full, acc, f32=(name == "f32"))


@pytest.mark.parametrize("cap", [50, 1100])
def test_batches_of_three_sizes_and_a_float32_pair_in_place(c, banks, cap):
    """Three integer pairs of three sizes share a launch; then the same with the float32 pair in the middle, which runs
    synchronously, in place.  Host and device outputs."""
    import torch
    sizes = [("planted", NQ, NT), ("planted", 300, 500), ("far", 1000, 260)]
    for names in (sizes, [sizes[1], ("f32", NQ, NT), sizes[2]]):
        pairs = [banks(*s) for s in names]
        for tau in sorted({TAU[s[0]] for s in names}):          # one threshold per call: every pair's list at that threshold
            want = [_expect(*s, tau=tau)[1] for s in names]
            assert any(len(w[0]) > 50 for w in want)
            outs = [_host_out(c, cap, True) for _ in pairs]
            cnts = [c.pinned_empty(1, np.int64) for _ in pairs]
            for cnt in cnts:
                cnt[0] = SENT
            c.match_accepted_batch(pairs, tau, outs, cnts)
            c.sync()
            for out, cnt, w, s in zip(outs, cnts, want, names):
                _check_host(out, cnt[0], w, cap, "match_accepted_batch %r tau=%g" % (s, tau))
            rows, counts = _dev_buffers(c, cap, len(pairs))
            torch.cuda.synchronize()
            hcs = c.pinned_empty(len(pairs), np.int64)
            hcs[:] = SENT
            c.match_accepted_dev_batch(pairs, tau, rows.data_ptr(), counts.data_ptr(), cap, h_counts=hcs)
            c.sync()
            for k, (w, s) in enumerate(zip(want, names)):
                _check_dev(rows[k], counts[k], w, cap, "match_accepted_dev_batch %r tau=%g" % (s, tau))
                assert int(hcs[k]) == len(w[0])


def _nothing():
    return (np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.float32), np.empty(0, np.float64))


def test_tau_zero_accepts_nothing(c, banks):
    full, acc = _expect("planted", tau=0.0)
    assert len(acc[0]) == 0 and not full[3].any()
    qb, tb = banks("planted")
    _all_deliveries(c, qb, tb, 0.0, full, acc, f32=False)


def test_empty_train_bank_gives_no_match(c, banks):
    qb, _ = banks("planted")
    tb = c.bank(np.zeros((0, 128), np.uint8))
    full = (np.full(NQ, -1, np.int32), np.full(NQ, np.inf, np.float32), np.full(NQ, np.nan), np.zeros(NQ, bool))
    _all_deliveries(c, qb, tb, TAU["planted"], full, _nothing(), f32=False)
    tidx, dist = c.xcheck1(qb, tb)
    assert _same(tidx, full[0]) and _same(dist, full[1])


def test_empty_query_bank_touches_nothing_but_the_count(c, banks):
    _, tb = banks("planted")
    qb = c.bank(np.zeros((0, 128), np.uint8))
    _all_deliveries(c, qb, tb, TAU["planted"], None, _nothing(), f32=False)


@pytest.mark.parametrize("name", ["planted", "far", "f32", "bin"])
def test_xcheck1_host_and_device_forms(c, banks, name):
    import torch
    if name == "bin":
        rng = np.random.default_rng(23)
        Q, T = rng.integers(0, 256, (NQ, 32), dtype=np.uint8), rng.integers(0, 256, (NT, 32), dtype=np.uint8)
        T[:200] = Q[100:300]
        T[:200, 0] ^= rng.integers(0, 4, 200, dtype=np.uint8)
        qb, tb = c.bank_binary(Q), c.bank_binary(T)
        otidx, odist = hamming_ref.xcheck(Q, T)
    else:
        qb, tb = banks(name)
        otidx, odist = _pair(name)[3]
    tidx, dist = c.xcheck1(qb, tb)
    assert _same(tidx, np.asarray(otidx, np.int32)) and _same(dist, np.asarray(odist, np.float32))
    assert (tidx >= 0).sum() > 100
    dev = torch.device("cuda", c.device)
    d_tidx = torch.full((NQ + 3,), SENT, dtype=torch.int32, device=dev)
    d_dist = torch.full((NQ + 3,), float(SENT), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.xcheck1_dev(qb, tb, d_tidx.data_ptr(), d_dist.data_ptr())
    c.sync()
    assert _same(d_tidx.cpu().numpy()[:NQ], tidx) and _same(d_dist.cpu().numpy()[:NQ], dist)
    assert (d_tidx.cpu().numpy()[NQ:] == SENT).all() and (d_dist.cpu().numpy()[NQ:] == SENT).all()


@pytest.mark.parametrize("call", ["xcheck1", "match_accepted", "match_accepted_async"])
def test_stats_account_one_call_and_every_pair(c, banks, call):
    qb, tb = banks("planted")
    every = c.get_option("async_time_every")
    c.set_option("async_time_every", 1)          # (every enqueue-only call carries its events: the accounting is exact)
    try:
        c.sync()
        before = c.stats()
        if call == "xcheck1":
            c.xcheck1(qb, tb)
        elif call == "match_accepted":
            c.match_accepted(qb, tb, TAU["planted"])
        else:
            out, cnt = _host_out(c, NQ, True), c.pinned_empty(1, np.int64)
            c.match_accepted_async(qb, tb, TAU["planted"], out, cnt)
        c.sync()
        after = c.stats()
    finally:
        c.set_option("async_time_every", every)
    assert after["calls"] - before["calls"] == 1
    assert after["pairs"] - before["pairs"] == NQ * NT
