"""Run the reference's solver, simulator and accessor once under AddressSanitizer + UBSan for the twelve example models
(TEST INFRASTRUCTURE; host code, CPU only) and print what the sanitizers report.

    python oracle/sanitize_ref.py [model ...]

Each gateway is linked with the stand-alone driver oracle/mexhost/ref_main.c, so the sanitizer runtime sits in the program;
its inputs are written by the ordinary build (ref_save) and its outputs are compared with the ordinary build's, byte for byte.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests', 'golden'))
import build_ref  # noqa: E402
import ref_harness  # noqa: E402
import make_golden_ref as G  # noqa: E402


def run(name, tmp):
    m = G.MODELS[name]()
    R = ref_harness.Reference(m)
    progs = build_ref.build_sanitized(m)
    sol = R.solve()
    init = G.init_rows(m)
    rs = G.randstream(m, init)
    jobs = {'ref_solver.so': (3, lambda h: [R._model(h)]),
            'ref_simulator.so': (1, lambda h: [R._model(h, sol=sol, init=init, randstream=rs), h.lib.mxCreateDoubleScalar(0.0)])}
    for k, (sw, args) in enumerate(G.call_cases(m, sol.nt, m.nst, m.nd)):
        jobs['ref_call.so#%d' % k] = (1, lambda h, sw=sw, args=args: [R._model(h, sol=sol), h.lib.mxCreateDoubleScalar(float(sw)), h.double(args)])
    reports = []
    for job, (nlhs, mk) in jobs.items():
        lib = job.split('#')[0]
        pre = os.path.join(tmp, '%s_%s' % (name, job.replace('#', '_')))

        def work():
            h = ref_harness._Host(R.libs[lib])
            h.lib.ref_save.argtypes, h.lib.ref_save.restype = [C.c_void_p, C.c_char_p], C.c_int
            ins = mk(h)
            for i, a in enumerate(ins):
                assert h.lib.ref_save(a, ('%s.in%d' % (pre, i)).encode()) == 0
            rc, out, msg, warn, nwarn = h.run(nlhs, ins)
            for i in range(nlhs if rc == 0 else 0):
                assert h.lib.ref_save(out[i], ('%s.plain.%d' % (pre, i)).encode()) == 0
            return rc, len(ins)

        rc, nin = ref_harness._in_child(work)
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
        r = subprocess.run(['bash', '-c', 'ulimit -s unlimited; exec "$@"', 'sh', progs[lib], str(nlhs), pre + '.san'] +
                           ['%s.in%d' % (pre, i) for i in range(nin)], env=env, capture_output=True, text=True)
        same = all(open('%s.plain.%d' % (pre, i), 'rb').read() == open('%s.san.%d' % (pre, i), 'rb').read()
                   for i in range(nlhs if rc == 0 else 0)) if r.returncode == 0 else False
        found = [ln for ln in r.stderr.splitlines() if 'runtime error' in ln or 'ERROR: AddressSanitizer' in ln or 'SUMMARY' in ln]
        print('%-18s %-16s exit=%d outputs_equal=%s reports=%d' % (name, job, r.returncode, same, len(found)), flush=True)
        for ln in sorted(set(found))[:12]:
            print('     ' + ln[-230:])
        reports += found
    return reports


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as tmp:
        total = 0
        for name in (sys.argv[1:] or sorted(k for k in G.MODELS if not k.startswith('C5_'))):
            total += len(run(name, tmp))
        print('sanitizer reports in all: %d' % total)
