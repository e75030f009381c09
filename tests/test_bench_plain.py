"""The plain benchmark run (-m gpu): `bench.py --steps K --warmup W` times exactly K steps in one region, its line carries the headline
and nothing measured beside it, and --dump-outputs writes what the last timed step returned: the arrays the engine gives for that
step's inputs when the same call is made here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    out_dir = tmp_path / 'outputs'
    steps, warmup = 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d['steps'] == steps and d['warmup'] == warmup and d['timed_regions'] == 1 and len(d['region_ms']) == 1
    assert d['ms_per_step'] == pytest.approx(d['region_ms'][0] / steps, rel=1e-3)
    assert d['unit'] == 'rollouts/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert d['value'] == pytest.approx(128 * 1e3 / d['ms_per_step'], rel=1e-9) and d['value'] > 1000
    for key in ('cpu_baseline', 'roofline', 'kernels_one_step', 'extras'):
        assert key not in d, key
    # the last timed step is step k = W + K - 1 (noise stage k x depth) on the benchmark's own seeded inputs: the same call here
    import bench
    import daimc_amd
    R, D, S, k = 128, 5, 10, warmup + steps - 1
    m = daimc_amd.ActiveInferenceModel(10, 4, 0.0, 1.0, 1.0, device='cuda:0', seed=1, row_offset=0)
    m.reserve(R, D, S)
    o = bench.synth_frames(R // 4, torch.device('cuda:0'), seed=100).repeat_interleave(4, dim=0).contiguous()
    pi = torch.eye(4, device='cuda:0').repeat(R // 4, 1).contiguous()
    G, T, po1 = m.calculate_G_repeated(o, pi, steps=D, samples=S, stage=k * D)
    P, logP = m.action_posterior(G)
    want = {'sum_G': G, 'sum_terms': torch.stack(T), 'po1': po1, 'P': P, 'logP': logP}
    assert sorted(os.listdir(out_dir)) == sorted(n + '.npy' for n in want)
    for n, t in want.items():
        got = np.load(out_dir / (n + '.npy'))
        assert got.dtype == np.float32, n
        np.testing.assert_array_equal(got, t.cpu().numpy(), err_msg=n)
