"""One example through the harness build with the envelope step's throughput path on, reporting what the period's tail launch
(k_tp_tail) did: cells the path completed / left over, and the second-tier cells that gave up and were done in place.
    python run_emu_tp_tail.py NAME 'KWARGS'      (environment as for run_emu.py)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import run_emu  # noqa: E402

if __name__ == '__main__':
    from egdst_amd import examples
    name = sys.argv[1]
    kw = eval('dict(%s)' % (sys.argv[2] if len(sys.argv) > 2 else ''))
    san = os.environ.get('EMU_SANITIZE', 'address')
    ok, rep, sol, ref, s = run_emu.run(examples.REGISTRY[name](**kw), {'0': False}.get(san, san), int(os.environ.get('EMU_ENV_BS', '1')),
                                        bool(int(os.environ.get('EMU_PAR_BLOCKS', '0'))), int(os.environ.get('EMU_WAVE', '1')))
    first = (s.tp_stats()[0].tolist(), int(s.tp_inplace()[0]))
    rest, big = s.tp_tail_counts()
    s.solve(raise_on_error=False)   # the tickets and the counters are cleared once per solve: a second one counts the same
    again = (s.tp_stats()[0].tolist(), int(s.tp_inplace()[0]))
    print(name, 'ok=%s status=%d rows=%d/%d evals=%d/%d max_rel=%.2e' % (ok, sol.status, sol.total_rows(), ref.total_rows(), sol.nevals,
                                                                           ref.nevals, rep['max_rel']),
          'tp done/left/in place', first[0] + [first[1]], 'second solve', again[0] + [again[1]],
          'listed per period: left over', rest[0].tolist(), 'second tier', big[0].tolist())
