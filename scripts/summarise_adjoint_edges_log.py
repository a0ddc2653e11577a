"""The header of profiles/adjoint_mlp_edges_gpu_tests.txt from the output of

    pytest -m gpu -s -v tests/test_gpu_adjoint_fused_edges.py

usage: summarise_adjoint_edges_log.py RUNLOG [OLD_SUITE_LOG] [note ...] > profiles/adjoint_mlp_edges_gpu_tests.txt
Parses the line every segment comparison prints (tests/test_gpu_adjoint_fused_edges.py, _against_the_oracle): the worst deviation per kernel
geometry as a share of that case's bound, the grids exercised, the runs with rejected attempts; then the run itself.  Notes (the counts of
the deliberately wrong scratch builds) are appended to the header as given."""
import collections
import os
import re
import sys

run = open(sys.argv[1]).read()
rest = sys.argv[2:]
old = open(rest.pop(0)).read() if rest and os.path.exists(rest[0]) else None
pat = re.compile(r'^(?:\S+ )?(\S+?)( \([^)]*\))? \[k_adjoint_mlp<(\d+), (\d+), (\w+)>, dim (\d+), hidden (\d+), batch (\d+), G (\d+)\]: adj_y (\S+) adj_t (\S+) '
                 r'adj_params (\S+) \(bound (\S+)\); attempts (\d+) \(oracle (\d+)\), accepted (\d+)', re.M)
per, grids, rej = collections.defaultdict(list), set(), []
for m in pat.finditer(run):
    name, tag = m.group(1), m.group(2) or ''
    dp, hp, act = int(m.group(3)), int(m.group(4)), m.group(5)
    dev, bound = max(float(m.group(i)) for i in (10, 11, 12)), float(m.group(13))
    att, acc = int(m.group(14)), int(m.group(16))
    per[dp, hp].append((dev, bound, name + tag, (int(m.group(6)), int(m.group(7))), act, att != acc))
    grids.add(int(m.group(9)))
    if att != acc and not tag:
        rej.append('%s (%d of %d)' % (name, att - acc, att))
dyn = [tuple(float(x) for x in m.groups()) for m in re.finditer(r'dynamics f (\S+), vjp_y (\S+), vjp_params (\S+) \(bar', run)]
between = [float(x) for x in re.findall(r'against grid 1: (\S+)', run)]


def outcome(text):
    return [line for line in text.splitlines() if re.search(r'\d+ (passed|failed)', line)][-1].strip('= ')


print('# pytest -m gpu -s -v tests/test_gpu_adjoint_fused_edges.py on the MI355X (%d compute units): %s' % (max(grids), outcome(run)))
if old is not None:
    print('# pytest -m gpu tests/test_gpu_adjoint_fused.py (the older suite of this kernel) next to it: %s' % outcome(old))
print('# %d segment comparisons against the numpy oracle; figures: max|got - ref| / (1 + |ref|) against the float64 oracle run on the float32-rounded inputs,'
      % sum(len(v) for v in per.values()))
print('# worst of adj_y, adj_t, adj_params; bound of a case: 4 x max(E32, bands.case_ceiling(attempts)); attempt / accept counts: the float32 oracle run\'s in every comparison')
print('#')
print('# worst deviation per geometry (by share of the case\'s bound)')
for k in sorted(per):
    v = per[k]
    w = max(v, key=lambda r: r[0] / r[1])
    print('k_adjoint_mlp<%2d, %3d>  %3d comparisons, (dim, hidden) %s, activations %s  worst %.3e (%s, bound %.3e: %.2f of it)  runs with rejected attempts %d'
          % (k[0], k[1], len(v), sorted({r[3] for r in v}), sorted({r[4] for r in v}), w[0], w[2], w[1], w[0] / w[1], sum(r[5] for r in v)))
print('#')
print('# one evaluation of the augmented dynamics against the float64 restatement (%d cases, bar 3e-6 of max |ref|): worst f %.3e, vjp_y %.3e, vjp_params %.3e'
      % ((len(dyn),) + tuple(max(d[i] for d in dyn) for i in range(3))))
print('# grids exercised (workgroups): %s; grid overrides 1, 2, 5, 24: the results differ from grid 1\'s by at most %.3e' % (sorted(grids), max(between)))
print('# runs with rejected attempts: %s' % ', '.join(rej))
for note in rest:
    print('# ' + note)
print('#')
print('# the run')
run = re.sub(r' ?/\S+amdgpu\.ids: No such file or directory', '', run)                    # (libdrm's complaint on a headless machine)
print(re.sub(r'^(platform|rootdir|plugins|cachedir).*\n', '', run, flags=re.M))
