# -*- coding:utf-8 -*-
"""References for training.KerasAdam(exact_rows=True) (csrc/adam_exact.hip), numpy only:
  * `dense_adam_step`: keras.optimizers.Adam's step over a WHOLE table in float64 from the densified gradient (duplicate
    lookups summed, rows that were not looked up take the step with gradient 0);
  * `idle_steps_f32`: a float32 mirror of the catch-up routine (adam_idle_steps) in its operation order — numpy rounds every
    float32 operation and contracts nothing — with the early exit switchable;
  * `idle_steps_f64`: the same idle steps one by one in float64, powers by `**`."""
import numpy as np

F32 = np.float32
EXIT = F32(2.0 ** -26)


def dense_adam_step(p, m, v, rows, vals, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """step t (1-based) on float64 arrays [V, D], in place; rows int [n] (-1 or >= V: skipped), vals [n, D]"""
    g = np.zeros_like(p)
    rows = np.asarray(rows).reshape(-1)
    ok = (rows >= 0) & (rows < p.shape[0])
    np.add.at(g, rows[ok], np.asarray(vals, dtype=np.float64).reshape(len(rows), -1)[ok])
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m *= b1
    m += (1.0 - b1) * g
    v *= b2
    v += (1.0 - b2) * g * g
    p -= lr_t * m / (np.sqrt(v) + eps)
    return p, m, v


def idle_steps_f32(p, m, v, s, k, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, early_exit=True):
    """elements (p, m, v) current through step s pay k idle steps -> (p, m, v, trips): float32 arrays of the broadcast shape
    and the number of loop trips each element made.  s, k: ints or int arrays."""
    p, m, v, s, k = np.broadcast_arrays(np.asarray(p, dtype=F32), np.asarray(m, dtype=F32), np.asarray(v, dtype=F32),
                                        np.asarray(s, dtype=np.int64), np.asarray(k, dtype=np.int64))
    p, m, v = p.copy(), m.copy(), v.copy()
    lr, b1, b2, eps = F32(lr), F32(b1), F32(b2), F32(eps)
    one = F32(1)
    with np.errstate(all='ignore'):
        c1, c2 = np.power(b1, s.astype(F32)), np.power(b2, s.astype(F32))
        paid = np.full(p.shape, -1, dtype=np.int64)
        trips = np.zeros(p.shape, dtype=np.int64)
        for j in range(int(k.max()) if k.size else 0):
            live = (paid < 0) & (j < k)
            if not live.any():
                break
            c1, c2 = c1 * b1, c2 * b2
            lr_t = lr * np.sqrt(one - c2) / (one - c1)
            mn, vn = b1 * m, b2 * v
            term = lr_t * mn / (np.sqrt(vn) + eps)
            pn = p - term
            stop = term == 0
            if early_exit:
                stop = stop | ((pn == p) & (np.abs(term) < EXIT * np.abs(pn)))
            else:
                stop = np.zeros_like(stop)
            m, v, p = np.where(live, mn, m), np.where(live, vn, v), np.where(live, pn, p)
            trips += live
            paid = np.where(live & stop, j + 1, paid)
        rest = np.where(paid < 0, 0, k - paid)
        owe = rest > 0
        m = np.where(owe, m * np.power(b1, rest.astype(F32)), m)
        v = np.where(owe, v * np.power(b2, rest.astype(F32)), v)
    return p, m, v, trips


def idle_steps_f64(p, m, v, s, k, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """the same k idle steps, each one taken, in float64 (from the float32 inputs)"""
    p, m, v, s, k = np.broadcast_arrays(np.asarray(p, dtype=F32).astype(np.float64), np.asarray(m, dtype=F32).astype(np.float64),
                                        np.asarray(v, dtype=F32).astype(np.float64), np.asarray(s, dtype=np.int64),
                                        np.asarray(k, dtype=np.int64))
    p, m, v = p.copy(), m.copy(), v.copy()
    lr, b1, b2, eps = (float(F32(x)) for x in (lr, b1, b2, eps))
    for j in range(int(k.max()) if k.size else 0):
        live = j < k
        t = (s + j + 1).astype(np.float64)
        lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        mn, vn = b1 * m, b2 * v
        pn = p - lr_t * mn / (np.sqrt(vn) + eps)
        m, v, p = np.where(live, mn, m), np.where(live, vn, v), np.where(live, pn, p)
    return p, m, v
