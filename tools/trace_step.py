"""Prints the kernels of one train() step of a rocprofv3 --kernel-trace CSV in launch order, with durations and the gaps between them.
usage: python tools/trace_step.py <kernel_trace.csv> [step | first-kernel-substring]      step: 0 = the first train() of the trace (the one that counts the corpus' classes), -1 = the last (default)
A step begins with its order-1 kernels: uni_finish_kernel and the uni_* counting kernels in front of it, which only a context's first run on a corpus launches."""
import csv, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r['Start_Timestamp']))
arg = sys.argv[2] if len(sys.argv) > 2 else '-1'
def short(r): return r['Kernel_Name'].split('(')[0].replace('colibri::', '').replace('void ', '')
starts = []
if arg.lstrip('-').isdigit():
    which = int(arg)
    for i, r in enumerate(rows):
        if short(r).startswith('uni_finish_kernel'):
            while i > 0 and short(rows[i - 1]).startswith('uni_'): i -= 1
            starts.append(i)
else:  # (a kernel's name: the steps begin where it is launched — the sharded trainers' steps, tools/trace_shard.sh)
    which = -1
    starts = [i for i, r in enumerate(rows) if arg in r['Kernel_Name']]
i0 = starts[which]
nxt = [s for s in starts if s > i0]
step = rows[i0:(nxt[0] if nxt else len(rows))]
end = next((k for k, r in enumerate(step) if 'export_len' in r['Kernel_Name']), len(step))
step = step[:end]
t0 = int(step[0]['Start_Timestamp']); prev_end = t0; total = 0.0
for r in step:
    s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
    print('%9.1f us  +%6.1f gap  %8.1f us  %s' % ((s - t0) / 1e3, (s - prev_end) / 1e3, (e - s) / 1e3, short(r)[:64]))
    total += (e - s) / 1e3; prev_end = e
print('kernels %.1f us, span %.1f us' % (total, (prev_end - t0) / 1e3))
