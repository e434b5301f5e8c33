"""The eta ladder of tests/test_gpu_train_derivative_ends.py, measured again: for every direction of
derivative_cases.END_DIRECTIONS and every rung 2^-a ... 2^-b the two metrics of the derivative check (rho: forward passes only,
the instrument; r: the gradient under test), how far the step moves the loss and the seconds the four passes took; then, per
stage and kind of variable, the largest rho of its directions at every rung and the rung the module's rule chooses -- from the
starting rung down while that largest rho still falls -- and the BAR the rule gives (the project's 8.5e-3 where 4 x the
largest rho at the chosen rungs is within it, else 4 x that rho; above 2e-2 the rule has no answer).  r is printed and takes no
part in any choice.  With --step the three directions the module measures again after an optimizer step are laddered at the
stepped point as well.  Run it on the GPU when a kernel of the training chain changes, and carry the tables into the test
module's docstring and DESIGN.md 4.39:

    python tools/derivative_ladder.py [--rungs 6:22] [--step]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'x-detector_amd'), ROOT]


PROJECT_BAR, CAP = 8.5e-3, 2e-2
START = {'kernels': 18, 'gamma/beta': 16, 'biases': 6}               # tests/test_gpu_train_derivative.py's rungs


def ladder(E, DC, chain, directions, rungs, title):
    at = E.loss_at(chain)
    table = {}
    print('\n%s: L = %.6f' % (title, chain.L0))
    print('%-42s %6s %9s %9s %9s %7s' % ('direction', 'eta', 'rho', 'r', '|dL|/L', 's'))
    for d in directions:
        for e in rungs:
            t0 = time.time()
            m = DC.measure(at, chain.x, chain.g, d.variables, 2.0 ** -e)
            table[d.name, e] = m
            print('%-42s 2^-%-3d %9.2e %9.2e %9.2e %7.2f' % (d.name, e, m.rho, m.r, m.dL / abs(m.L), time.time() - t0), flush=True)
    assert at({}) == chain.L0, 'the base point was not restored'
    return table


def choose(table, directions, rungs):
    """per stage and kind: the largest rho of its directions per rung, and the rung the rule takes; the same per kind over all
    stages is printed beside it (one eta per kind, the older module's form)"""
    chosen = {}
    stages = sorted({d.stage for d in directions}, key=[d.stage for d in directions].index)
    for kind in ('kernels', 'gamma/beta', 'biases'):
        for stage in stages + [None]:
            names = [d.name for d in directions if d.kind == kind and stage in (d.stage, None)]
            if not names:
                continue
            worst = {e: max(table[n, e].rho for n in names) for e in rungs}
            e = START[kind] if START[kind] in worst else rungs[0]
            while e + 1 in worst and worst[e + 1] < worst[e]:
                e += 1
            if stage is not None:
                chosen[stage, kind] = e
            print('%-10s %-11s 2^-%-3d %s' % (stage or 'all stages', kind, e, '   '.join('2^-%d %.1e' % (k, worst[k]) for k in rungs)))
    return chosen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rungs', default='6:22', help='a:b -> 2^-a ... 2^-b')
    ap.add_argument('--step', action='store_true', help='the three post-step directions at the stepped point too')
    args = ap.parse_args()
    a, b = (int(v) for v in args.rungs.split(':'))
    rungs = list(range(a, b + 1))
    import derivative_cases as DC
    import test_gpu_train_derivative_ends as E
    from xdet import weights as W
    t0 = time.time()
    chain = E.build_chain(W.make_lighthead_weights(1234))
    print('the detector and the base pass: %.1f s' % (time.time() - t0))
    table = ladder(E, DC, chain, DC.END_DIRECTIONS, rungs, 'the base point')
    print('\nlargest rho of the kind per rung, and the rung chosen')
    chosen = choose(table, DC.END_DIRECTIONS, rungs)
    top = max(table[d.name, chosen[d.stage, d.kind]].rho for d in DC.END_DIRECTIONS)
    bar = PROJECT_BAR if 4 * top <= PROJECT_BAR else 4 * top
    print('largest rho at the chosen rungs %.3e -> BAR %.3e%s' % (top, bar, '' if bar <= CAP else ' (ABOVE THE CAP %.0e)' % CAP))
    print('\nat the chosen rungs')
    for d in DC.END_DIRECTIONS:
        m = table[d.name, chosen[d.stage, d.kind]]
        print('%-42s 2^-%-3d %9.2e %9.2e %9.2e' % (d.name, chosen[d.stage, d.kind], m.rho, m.r, m.dL / abs(m.L)))
    if args.step:
        stepped, _ = E.step_chain(chain)
        print('\nthe step moved L from %.6f to %.6f' % (chain.L0, stepped.L0))
        after = [E.by_name(n) for n in E.AFTER_A_STEP]
        t2 = ladder(E, DC, stepped, after, rungs, 'after one step')
        print('\nafter one step, at the rungs chosen at the base point')
        for d in after:
            m = t2[d.name, chosen[d.stage, d.kind]]
            print('%-42s 2^-%-3d %9.2e %9.2e %9.2e' % (d.name, chosen[d.stage, d.kind], m.rho, m.r, m.dL / abs(m.L)))


if __name__ == '__main__':
    main()
