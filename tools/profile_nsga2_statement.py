"""Writes profiles/nsga2_statement.txt: what the numpy statement of smart_nsga2_step_hip (oracle/analyses/nsga2.py) reaches on
the two-point problem over six seeds, and the thresholds tests/test_nsga2_host.py takes from it (the worst seed times two).
No device needed.  `python tools/profile_nsga2_statement.py`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np                      # noqa: E402
import cases_nsga2 as st                # noqa: E402


def main():
    c = st.CONVERGENCE
    lines = ['NSGA-II, the numpy statement (oracle/analyses/nsga2.py) on the two-point problem: two objectives, the negated',
             'squared distances to two points of the unit box; the Pareto set is the segment between them.',
             'd = %d, N = %d, %d generations, f = 0.5, CR = 0.9, b* = 1e-6, Philox draws, uniform initial population of the seed.'
             % (c['d'], c['N'], c['generations']),
             '', 'seed  mean distance to the segment   largest gap along it   outermost projection to the nearer end',
             '      before      after                before      after      after']
    worst = np.zeros(3)
    for seed in c['seeds']:
        before, after, best = st.convergence_run(seed)
        assert (np.diff(best, axis=0) >= 0).all()
        worst = np.maximum(worst, after)
        lines.append('%4d  %.6f    %.6f             %.6f    %.6f   %.6f' % (seed, before[0], after[0], before[1], after[1],
                                                                           after[2]))
    lines += ['', 'worst of the six seeds:   distance %.6f   gap %.6f   ends %.6f' % tuple(worst),
              'thresholds (worst x 2):   distance %.6f   gap %.6f   ends %.6f' % tuple(2.0 * worst),
              'The best key of either objective never fell from one generation to the next, in any seed.']
    text = '\n'.join(lines) + '\n'
    with open(os.path.join(ROOT, 'profiles', 'nsga2_statement.txt'), 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()
