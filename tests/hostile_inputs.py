"""Input generators shared by the CPU and GPU parity tests (no test functions here)."""
import numpy as np


def hostile_matrix(rnd, n, dtype):
    """(rate, next, hops) of hostile_matrix_mix."""
    return hostile_matrix_mix(rnd, n, dtype)[:3]


def hostile_matrix_mix(rnd, n, dtype):
    """(rate, next, hops, heavy).  Entries drawn from a pool of awkward values: zeros of both signs, ties,
    subnormals, values that overflow when multiplied, infinities, NaN, negatives.  The diagonal is arbitrary too
    (the reference never reads or writes it, Algorithms.hs:54).  heavy: which of the two mixes was drawn."""
    fi = np.finfo(dtype)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 0.5, 0.5, 2.0, 0.25, 3.0, 1e-3, 7.0, fi.tiny, fi.tiny / 4,
                     fi.max / 2, fi.max, np.inf, -np.inf, np.nan, -1.0, -0.5, 1.5, 0.999], dtype=dtype)
    heavy = rnd.random() < 0.5          # half of the cases: mostly ordinary rates, a few oddities
    p = np.ones(len(pool))
    if heavy:
        p[2:11] = 12.0
    rate = rnd.choice(pool, size=(n, n), p=p / p.sum()).astype(dtype)
    nxt = np.where(rnd.random((n, n)) < 0.8, np.arange(n, dtype=np.int32)[None, :], -1).astype(np.int32)
    hops = (nxt >= 0).astype(np.int32)
    return np.ascontiguousarray(rate), np.ascontiguousarray(nxt), np.ascontiguousarray(hops), bool(heavy)


def market_rates(n_exch, n_ccy, seed, density=0.5):
    """The reference's own kind of graph: per-exchange quotes plus its built-in rate-1.0 edges
    between the same currency on two exchanges (Algorithms.hs:35) -- exact ties everywhere."""
    rnd = np.random.default_rng(seed)
    ccys = ["C%02d" % i for i in range(n_ccy)]
    price = dict(zip(ccys, 0.5 + 1.5 * rnd.random(n_ccy)))
    rates = {}
    for e in range(n_exch):
        exch = "X%02d" % e
        for i in range(n_ccy):
            for j in range(i + 1, n_ccy):
                if rnd.random() < density:
                    a, b = ccys[i], ccys[j]
                    rates[((exch, a), (exch, b))] = price[b] / price[a] * (0.97 + 0.03 * rnd.random())
                    rates[((exch, b), (exch, a))] = price[a] / price[b] * (0.97 + 0.03 * rnd.random())
    return rates
