"""The schedule-driven splat's instruction stream (unires_amd/csrc/splat2.hip, k_splat2): the build pads every tile to
whole batches of instructions and stores, per batch, the ring slot of each instruction's first segment entry and
whether the segment ring moves on before it (splat2.hpp, kS2Batch).  On a mid-size rotated thick-z operator (the
bench's form, conv_up along z) the push and the matvec are bit-identical from launch to launch and under the
channel-stream sizing of the persistent grid, and agree with the round-1 push (UNIRES_NO_SPLAT2=1, a fresh process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import hashlib, json, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from tests.helpers import make_problem, gpu_structs
from unires_amd._project import _channel_plan
prob = make_problem(seed=23, dim_y=(96, 88, 120), n_channels=1, thick=6, regime='sr', rot=0.12, trans=2.5,
                    thick_axes=[2])
xg, yg, sett = gpu_structs(prob, 'cuda:0')
plan = _channel_plan(xg[0], yg[0], prob['method'], True)
info = plan.repeat_info(0)
g = torch.Generator().manual_seed(7)
p = (torch.rand(prob['dim_y'], generator=g) * 100).to('cuda:0')
v = (torch.rand(tuple(xg[0][0].dat.shape), generator=g) * 100).to('cuda:0')
h = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
out = {'axis': info['splat2_axis'], 'At': [], 'mv': []}
for conc in (1, 3, 1):
    plan.set_concurrency(conc)
    for _ in range(3):
        At = plan.proj_apply(0, 'At', v)
        mv = plan.matvec(p, 0.9, 0.006)
        torch.cuda.synchronize()
        out['At'].append(h(At)), out['mv'].append(h(mv))
np.savez(sys.argv[1] + '.npz', At=At.cpu().numpy(), mv=mv.cpu().numpy())
json.dump(out, open(sys.argv[1], 'w'))
'''


def _child(tmp_path, tag, extra):
    path = str(tmp_path / ('s2_%s.json' % tag))
    env = {k: v for k, v in os.environ.items() if k != 'UNIRES_NO_SPLAT2'}
    r = subprocess.run([sys.executable, '-c', _CHILD % dict(root=ROOT), path], env=dict(env, **extra),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.load(open(path)), np.load(path + '.npz')


def test_stream_is_bit_reproducible_and_matches_the_round1_push(tmp_path):
    res, arr = _child(tmp_path, 'splat2', {})
    assert res['axis'] == 2, res['axis']
    # every launch, every grid sizing: the same bits
    assert len(set(res['At'])) == 1 and len(set(res['mv'])) == 1, res
    _, rarr = _child(tmp_path, 'round1', {'UNIRES_NO_SPLAT2': '1'})
    for k in ('At', 'mv'):
        assert rel_err(torch.from_numpy(arr[k]), torch.from_numpy(rarr[k])) < 2e-5, k
