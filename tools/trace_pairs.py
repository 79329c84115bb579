"""Per queue of the last solve in a rocprofv3 kernel trace csv: every k_tp_big launch paired with the k_envelope launch that follows
it on the same queue, the sums of their durations and of min(pair) -- the most that running the two as one launch can save --
and the launches of k_tp_tail, the one launch they became (profiles/r08_tp_tail_C2_ndraw4096.txt).
    python tools/trace_pairs.py DIR [NSOLVES]
NSOLVES: solves in the trace (bench.py: warm-up + steps); the last 1 / NSOLVES of the kernels, by start time, are taken as the
last solve, as tools/trace_queues.py does -- a few launches more or less where the solves are not equally long."""
import collections
import csv
import glob
import sys


def duration_us(row):
    return (int(row['End_Timestamp']) - int(row['Start_Timestamp'])) / 1e3


d = sys.argv[1]
nsolves = int(sys.argv[2]) if len(sys.argv) > 2 else 5
f = glob.glob(d + '/**/*_kernel_trace.csv', recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if r['Kernel_Name'].startswith('k_')]
rows.sort(key=lambda r: int(r['Start_Timestamp']))
rows = rows[len(rows) - len(rows) // nsolves:]
qk = 'Queue_Id' if 'Queue_Id' in rows[0] else [k for k in rows[0].keys() if 'ueue' in k][0]
by = collections.defaultdict(list)
for r in rows:
    by[r[qk]].append(r)
for q, rs in sorted(by.items()):
    pairs = [(duration_us(a), duration_us(b)) for a, b in zip(rs, rs[1:])
             if a['Kernel_Name'].startswith('k_tp_big') and b['Kernel_Name'].startswith('k_envelope')]
    tail = [duration_us(r) for r in rs if r['Kernel_Name'].startswith('k_tp_tail')]
    span = (max(int(r['End_Timestamp']) for r in rs) - min(int(r['Start_Timestamp']) for r in rs)) / 1e6
    busy = sum(duration_us(r) for r in rs) / 1e3
    print('queue %s: %d kernels, span %.1f ms, busy %.1f ms; %d pairs: sum k_tp_big %.2f ms, sum k_envelope %.2f ms, sum of min %.2f ms; k_tp_tail n=%d sum %.2f ms'
          % (q, len(rs), span, busy, len(pairs), sum(a for a, _ in pairs) / 1e3, sum(b for _, b in pairs) / 1e3,
             sum(min(p) for p in pairs) / 1e3, len(tail), sum(tail) / 1e3))
