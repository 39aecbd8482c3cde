#!/usr/bin/env python3
"""Every value of the golden model cases that misses its direct bound in tests/test_oracle_golden.py on THIS CPU, with the
two quantities the arbitration of that test decides on: how far the fp32 oracle and the golden vector each are from the
oracle evaluated in float64, their ratio (against ARB_SLACK) and the golden value's distance against its GOLDEN_F64 bound.

    python tools/oracle_arbitration.py                                 # this CPU's default MKL code path
    MKL_ENABLE_INSTRUCTIONS=AVX2 python tools/oracle_arbitration.py    # (also SSE4_2; MKL_CBWR=COMPATIBLE)

The last line is the largest ratio and the largest golden distance (as a fraction of its bound) over all cases."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import test_oracle_golden as T  # noqa: E402
from helpers import golden_cases  # noqa: E402


def main():
    rows = []

    def record(self, key, got, floor, miss):
        if self.f64 is None:
            self.f64 = T._f64_case(self.g)
        got = torch.as_tensor(got.detach() if torch.is_tensor(got) else got, dtype=torch.float64).reshape(-1)
        ref = torch.as_tensor(self.g.z[key], dtype=torch.float64).reshape(-1)
        exact = self.f64[key].detach().double().reshape(-1)
        e_orc, e_ref = (got - exact).abs().max().item(), (ref - exact).abs().max().item()
        keys = T.ILL_CONDITIONED.get(self.name, ())
        rows.append((self.name, key, keys is None or key in keys, (e_orc - floor) / max(e_ref, 1e-300), e_orc, e_ref,
                     e_ref / T._golden_f64_bound(self.g, key, self.scale)))
    T._Arbiter.__call__ = record
    for name in golden_cases('model'):
        T.test_model_matches_reference(name)
    for name, key, named, ratio, e_orc, e_ref, gfrac in rows:
        print('%-28s %-46s %-7s ratio %5.2f  oracle-f64 %.2e  golden-f64 %.2e  golden/bound %.2f'
              % (name, key, 'named' if named else 'UNNAMED', ratio, e_orc, e_ref, gfrac))
    print('values beyond their direct bound: %d (%d outside ILL_CONDITIONED); largest ratio %.2f (ARB_SLACK %.1f); '
          'largest golden/bound %.2f' % (len(rows), sum(not r[2] for r in rows), max([r[3] for r in rows] or [0.0]), T.ARB_SLACK,
                                          max([r[6] for r in rows] or [0.0])))


if __name__ == '__main__':
    main()
