#!/usr/bin/env python
"""Evidence for the folded form of the rare bond-type channels in the strip forward,
run ON THE GPU BOX from the repository root:

    python tools/strip_rare_profile.py OUTDIR PARENT_TREE [RUNS]

PARENT_TREE is a built checkout of the parent commit (its own `build()` done).  Every step is a fresh
process under a time limit; the first failing step ends the script.

  1. `bench.py --gpus 1 --steps 50 --warmup 10`, parent and this tree alternating, RUNS (3) times each
  2. one `rocprofv3 --kernel-trace --stats` run of that command per tree
  3. `rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F32` ALONE on this tree (`--steps 7 --warmup 2`)
  4. `bench.py --full --no-secondary --cpu-reps 1` on this tree (parity gate), dumping the timed plan

Writes OUTDIR/strip_rare_bench.json, strip_rare_pmc.json and the two kernel tables (copy them to
profiles/ under the round's name).  The touched rows of the timed batch (seed 0) are derived on the host
from the oracle's L4 (utils/flop_model.py: touch_masks, strip_touch_counts)."""
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BENCH = ['bench.py', '--gpus', '1', '--steps', '50', '--warmup', '10']
COUNTER = 'SQ_INSTS_VALU_MFMA_MOPS_F32'
QM8 = dict(num_bond_type=6, short_diffusion_dist=[], long_diffusion_dist=[1, 2, 3, 5, 7, 10, 20, 30],
           num_eig_vec=20, input_dim=64, hidden_dim=[128] * 7, num_layer=7)


def run(cmd, cwd, limit, env=None):
  """-> stdout of a step; a failing step (or one past its time limit) ends the script."""
  p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, cwd=cwd, env=env, stdout=subprocess.PIPE,
                     stderr=subprocess.PIPE, text=True)
  if p.returncode != 0:
    sys.exit('step failed (rc %d): %s\n%s' % (p.returncode, ' '.join(cmd), p.stderr[-2000:]))
  return p.stdout


def bench_line(cwd, extra=(), limit=240, env=None):
  return json.loads(run([sys.executable] + BENCH + list(extra), cwd, limit, env).strip().splitlines()[-1])


def short(name):
  return name.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0]


def kernel_stats(cwd, d):
  run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--', sys.executable] + BENCH,
      cwd, 300)
  f = glob.glob(d + '/**/*kernel_stats.csv', recursive=True)[0]
  return f, {short(r['Name']): {'calls': int(r['Calls']), 'avg_us': round(float(r['AverageNs']) / 1e3, 2),
                                'pct': float(r['Percentage'])} for r in csv.DictReader(open(f))}


def main():
  out, parent = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
  runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
  os.makedirs(out, exist_ok=True)
  rec = {'command': ' '.join(BENCH), 'order': 'parent, change, alternating',
         'parent': {'ms_per_step': [], 'forward_launch_ms': []}, 'change': {'ms_per_step': [], 'forward_launch_ms': []}}
  for _ in range(runs):
    for key, cwd in (('parent', parent), ('change', ROOT)):
      r = bench_line(cwd)
      rec[key]['ms_per_step'].append(r['ms_per_step'])
      rec[key]['forward_launch_ms'].append(r['config']['stage_ms']['lanczosnet_forward'])
  p, c = rec['parent'], rec['change']
  rec['gain'] = {'slowest_change_ms': max(c['ms_per_step']), 'fastest_parent_ms': min(p['ms_per_step']),
                 'step_ratio': round(float(np.mean(c['ms_per_step']) / np.mean(p['ms_per_step'])), 4),
                 'forward_ratio': round(float(np.mean(c['forward_launch_ms']) / np.mean(p['forward_launch_ms'])), 4)}
  rec['kernel_trace_stats'] = {'command': 'rocprofv3 --kernel-trace --stats -- python ' + ' '.join(BENCH)}
  for key, cwd in (('parent', parent), ('change', ROOT)):
    f, table = kernel_stats(cwd, os.path.join(out, 'stats_' + key))
    shutil.copy(f, os.path.join(out, 'strip_rare_%skernel_stats.csv' % ('parent_' if key == 'parent' else '')))
    rec['kernel_trace_stats'][key] = table
  # the counter, alone
  d = os.path.join(out, 'pmc')
  run(['rocprofv3', '--pmc', COUNTER, '--output-format', 'csv', '-d', d, '--', sys.executable, 'bench.py',
       '--gpus', '1', '--steps', '7', '--warmup', '2'], ROOT, 300)
  rows = [r for r in csv.DictReader(open(glob.glob(d + '/**/*counter_collection.csv', recursive=True)[0]))
          if r['Counter_Name'] == COUNTER and 'lanczosnet_strip_kernel' in r['Kernel_Name']]
  vals = [float(r['Counter_Value']) for r in rows]
  # parity gate and the timed plan
  plan_file = os.path.join(out, 'strip_plan.npz')
  full = bench_line(ROOT, ('--full', '--no-secondary', '--cpu-reps', '1'), 600,
                    dict(os.environ, LNZ_BENCH_DUMP_PLAN=plan_file))
  rec['full_run_of_the_change'] = {
      'command': ' '.join(BENCH) + ' --full --no-secondary --cpu-reps 1', 'parity_rel_err': full['parity_rel_err'],
      'ms_per_step': full['ms_per_step'], 'roofline_kernel': full['roofline']['kernel'],
      'roofline_frac': full['roofline']['frac'],
      'roofline_frac_is': "the channel loop's instruction count (strip_mfma_issued) over the launch time: an "
                          'equivalent-work rate'}
  json.dump(rec, open(os.path.join(out, 'strip_rare_bench.json'), 'w'), indent=1)

  import oracle
  from lanczosnet_amd.synthetic import draw_batch
  from lanczosnet_amd.utils import flop_model as fm
  b = draw_batch(1024, seed=0)
  B, N = b['node_mask'].shape
  L = np.zeros((B, N, N, 7), np.float32)
  for i in range(B):
    n = int(b['n_nodes'][i])
    L[i, :n, :n] = oracle.laplacian_multi_l4(b['adjs'][i, :n, :n])
  plan = np.load(plan_file)
  counts = fm.strip_touch_counts(plan['strips'], fm.touch_masks(L, b['node_mask']), 7)
  strips = fm.strips_from_plan(plan['strips'], plan['ident'])
  m, o = fm.strip_rare_mfma_issued(strips, counts, QM8), fm.strip_mfma_issued(strips, QM8)
  fwd_ms = float(np.mean(c['forward_launch_ms']))
  tflops = m['flops_issued'] / (fwd_ms * 1e-3) / 1e12
  pmc = {'command': 'rocprofv3 --pmc %s -- python bench.py --gpus 1 --steps 7 --warmup 2 (the counter alone)' % COUNTER,
         'kernel': short(rows[0]['Kernel_Name']), 'launches': len(vals),
         COUNTER + '_per_launch': float(np.mean(vals)), 'per_launch_min': min(vals), 'per_launch_max': max(vals),
         'mfma_instruction': 'v_mfma_f32_16x16x4_f32', 'mfma_instructions_per_launch': float(np.mean(vals)) / 4.0,
         'plan': 'strip_plan.npz beside this file (strips, ident)',
         'touch_counts': 'touched rows of channels 2..6 per strip of that plan, seed-0 batch',
         'touch_counts_per_strip': [[int(x) for x in t] for t in counts],
         'model': {'strip_rare_mfma_issued': m['mfma_issued'], 'mops_counts': m['mops_counts'],
                   'channel_loop_mfma_issued': o['mfma_issued'],
                   'issued_over_channel_loop': round(m['mfma_issued'] / o['mfma_issued'], 4),
                   'rare_strips': m['rare_strips'], 'virtual_subtiles': m['virtual_subtiles'],
                   'per_wave_layer_worst': m['per_wave_layer_worst'],
                   'per_wave_layer_mean': round(m['per_wave_layer_mean'], 2)},
         'honest_issue_fraction': {
             'note': "issued MFMA flops of the folded form over the launch time and the fp32 matrix peak, next to "
                     "bench.py --full roofline.frac, which prices the channel loop's count",
             'forward_launch_ms': fwd_ms, 'issued_tflops': round(tflops, 2),
             'issued_frac_of_peak_157.3': round(tflops / 157.3, 4)}}
  text = json.dumps(pmc, indent=1)   # (a strip's five counts on one line)
  text = re.sub(r'\[\s+(\d+),\s+(\d+),\s+(\d+),\s+(\d+),\s+(\d+)\s+\]', r'[\1, \2, \3, \4, \5]', text)
  open(os.path.join(out, 'strip_rare_pmc.json'), 'w').write(text + '\n')
  print(json.dumps({'gain': rec['gain'], 'parity_rel_err': full['parity_rel_err'],
                    'counter': pmc[COUNTER + '_per_launch'], 'model': m['mops_counts']}))


if __name__ == '__main__':
  main()
