"""The bounds of discover.hip's pass epilogue emulated in numpy float32 against the contract's formulas
(tests/_discover_checks.py): random scan scores, error bounds e from 1e-30 to 2e-2 and fp32 scores anywhere within e of them,
at three magnitudes.  Asserts that every computed sig lies between its two ends, that a pair classified surely +1 / -1 has
that rank, and that every computed loss lies between its two ends (the 1 ulp reciprocal taken as 2.5e-7 relative, against
the bound); prints the smallest distance of a sig from its bound.  No GPU.
    python scripts/discover_bounds_check.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _discover_checks as dc  # noqa: E402

f = np.float32
rng = np.random.default_rng(0)
M = 2_000_000
def sd(x, ref): return (x - f(4e-7) * (f(1) + np.abs(ref))).astype(f)
def su(x, ref): return (x + f(4e-7) * (f(1) + np.abs(ref))).astype(f)
worst = 1e9
for e in (f(1e-30), f(1e-7), f(3e-6), f(1e-3), f(2e-2)):
    for scale in (1.0, 1e-3, 1e-6):
        # discovery sig: scan score t, true st anywhere within e
        t = (rng.uniform(-1.001, 1.001, M) * scale).astype(f)
        st = (t.astype(np.float64) + rng.uniform(-1, 1, M) * float(e)).astype(f)
        st = np.clip(st, (t.astype(np.float64) - float(e)), (t.astype(np.float64) + float(e))).astype(f)
        ok = np.abs(st.astype(np.float64) - t) <= float(e)
        s_lo = dc.sig((t - e).astype(f)); s_hi = dc.sig((t + e).astype(f))
        lo = sd(s_lo, s_lo); hi = su(s_hi, s_hi)
        v = dc.sig(st)
        assert (v[ok] >= lo[ok]).all() and (v[ok] <= hi[ok]).all(), ("sig", e, scale)
        worst = min(worst, float((v[ok] - lo[ok]).min()), float((hi[ok] - v[ok]).min()))
        # pair: a, b scan scores; sp, sn within e
        a = (rng.uniform(-1.001, 1.001, M) * scale).astype(f)
        b = (a + (rng.uniform(-1, 1, M) * max(scale * 1e-3, 4 * float(e))).astype(f)).astype(f)
        sp = (a.astype(np.float64) + rng.choice([-1, 1, 0.3, -0.7], M) * float(e)).astype(f)
        sn = (b.astype(np.float64) + rng.choice([-1, 1, 0.3, -0.7], M) * float(e)).astype(f)
        ok = (np.abs(sp.astype(np.float64) - a) <= float(e)) & (np.abs(sn.astype(np.float64) - b) <= float(e))
        d = (a - b).astype(f); e2 = f(2) * e
        plus = sd((d - e2).astype(f), d) > 0; minus = su((d + e2).astype(f), d) < 0
        assert (sp[ok & plus] > sn[ok & plus]).all() and (~(sp[ok & minus] > sn[ok & minus])).all(), ("rank", e, scale)
        # context term
        w = (f(2e-6) * (f(1) + np.abs(d))).astype(f)
        eps = f(np.finfo(f).eps)
        xl = (((d - e2).astype(f) - eps).astype(f) - w).astype(f); xh = (((d + e2).astype(f) - eps).astype(f) + w).astype(f)
        # 1-ulp reciprocal emulated pessimistically: exact quotient then +-2 ulp
        def fsa(x, sgn):
            q = (x.astype(np.float64) / (1.0 - x.astype(np.float64)))
            return (q + sgn * 2.5e-7 * np.abs(q)).astype(f)
        fl = np.where(xl >= 0, f(0), fsa(xl, -1) - f(1e-6)).astype(f)
        fh = np.where(xh >= 0, f(0), np.minimum(fsa(xh, +1) + f(1e-6), f(0))).astype(f)
        L = dc.context_loss(sp[None], sn[None])[0]
        assert (L[ok] >= fl[ok]).all() and (L[ok] <= fh[ok]).all(), ("loss", e, scale, np.nonzero(ok & ((L < fl) | (L > fh)))[0][:5])
print("bounds hold; smallest sig margin", worst)
