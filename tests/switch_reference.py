"""References for switches the library reads once per process (UNIRES_CG_TRIM, UNIRES_CG_START_FUSED): the test module
that needs one is run once as a child process with the switch set; there it computes every case of its ``reference()``
and saves the results, which the tests of the parent process then share."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def from_child(module, env, out_path):
    """Runs ``python -m <module> <out_path>`` with ``env`` added to the environment; returns what it saved."""
    e = dict(os.environ)
    e.update(env)
    # (the cases take seconds; the limit only keeps a child that hangs from holding the whole suite)
    r = subprocess.run([sys.executable, '-m', module, str(out_path)], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(str(out_path), weights_only=False)


def child_main(reference):
    """``if __name__ == '__main__'`` of such a module: ``reference(dev)`` -> dict, saved to argv[1].  (The library is the one the
    parent's ``lib`` fixture built.)"""
    out = reference(torch.device('cuda:0'))
    torch.cuda.synchronize()
    torch.save(out, sys.argv[1])


def switch_on(name):
    """Whether this process runs with the library's switch ``name`` on (they default to on; '0' turns one off)."""
    return not os.environ.get(name, '').startswith('0')


def cg_ends(plan):
    """(trimmed, start_fused) of the plan's last solve (``unires_plan_cg_ends``)."""
    import ctypes as C
    t, f = C.c_int32(-1), C.c_int32(-1)
    assert plan.lib.unires_plan_cg_ends(plan._h, C.byref(t), C.byref(f)) == 0
    return bool(t.value), bool(f.value)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))
