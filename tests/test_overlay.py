"""The `tt` package is an overlay: hot-path modules come from this repo, everything else from another `tt` package further down
sys.path (the reference checkout in a training setup).  The tests put a small stand-in of that lower package there: modules the
overlay must shadow refuse to import, the others mark themselves, and its host-side concat_frame is the oracle's numpy restatement."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, PKG, ROOT

LOWER = {
    "model.py": "raise ImportError('the overlay must shadow tt.model')\n",
    "optim.py": "raise ImportError('the overlay must shadow tt.optim')\n",
    "kaldi_io.py": "LOWER = True\n",
    "utils.py": "import sys\nsys.path.insert(0, %r)\nfrom oracle.frontend_oracle import concat_frame  # noqa: F401\n\n\n"
                "def init_logger(*args, **kwargs):\n    return 'lower init_logger'\n" % ROOT,
}


@pytest.fixture
def lower(tmp_path):
    """a directory holding the stand-in lower `tt` package, to go behind the overlay on PYTHONPATH"""
    (tmp_path / "tt").mkdir()
    for name, src in LOWER.items():
        (tmp_path / "tt" / name).write_text(src)
    return str(tmp_path)


def test_non_hot_path_modules_resolve_to_the_reference(lower):
    code = r"""
import sys
sys.dont_write_bytecode = True
import tt, tt.model, tt.encoder, tt.transformer, tt.utils
import tt.optim                                   # the overlay's (round 2): the reference's wrapper surface on the flat-buffer optimiser
import tt.kaldi_io                                # not part of the overlay -> the lower package's own file
assert tt.model.__file__.startswith(%r), tt.model.__file__
assert tt.kaldi_io.__file__.startswith(%r) and tt.kaldi_io.LOWER, tt.kaldi_io.__file__
assert tt.optim.__file__.startswith(%r), tt.optim.__file__
from tt.utils import AttrDict, look_ahead_mask, context_mask       # hot-path names: ours
assert AttrDict.__module__ == "tt.utils" and tt.utils.__file__.startswith(%r)
cfg = AttrDict(dict(type="sgd", lr=0.1, momentum=0.9, weight_decay=0.0, decay_ratio=0.5))
import torch
opt = tt.optim.Optimizer([torch.nn.Parameter(torch.zeros(3))], cfg)   # same constructor and counters as the reference's wrapper
opt.epoch(); opt.decay_lr()
assert abs(opt.lr - 0.05) < 1e-12 and opt.global_step == 1
assert tt.utils.init_logger() == "lower init_logger"                  # not part of the overlay -> served by the lower tt/utils.py
print("overlay ok")
""" % (PKG, lower, PKG, PKG)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + lower, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "overlay ok" in out.stdout


def test_host_side_feature_calls_reach_the_reference_inside_dataloader_workers(lower):
    """tt/dataset.py calls get_feature2 + concat_frame on numpy data inside AudioDataset.__getitem__, which train.py:174-184 runs in
    fork-started DataLoader workers after model.cuda(): those calls must never reach the HIP library.  Host data is served by the
    lower package's own numpy functions; the result equals the reference-run fixture."""
    code = r"""
import sys
sys.dont_write_bytecode = True
import numpy as np, torch
import torch.utils.data as D
import tt.utils as U
assert U.__file__.startswith(%r)
fz = dict(np.load(%r))                # read every array before the DataLoader forks: forked workers would share one open .npz handle

class DS(D.Dataset):
    def __len__(self): return 4
    def __getitem__(self, i):
        assert D.get_worker_info() is not None
        return torch.from_numpy(U.subsampling(U.concat_frame(fz["feat"], 3, 0), 3))

import ttmi
calls = []
real = ttmi.lib
ttmi.lib = lambda: calls.append(1) or real()          # (the forked workers inherit this; any use of the HIP library would be counted there, not here -
for batch in D.DataLoader(DS(), batch_size=2, num_workers=2):   # so the worker asserts by construction: a HIP call on a box without a GPU raises)
    for row in batch:
        assert np.array_equal(row.numpy(), fz["sub_3"])
assert np.array_equal(U.concat_frame(fz["feat"], 2, 1), fz["concat_2_1"])
assert U._reference_utils().__file__.startswith(%r)
print("workers ok")
""" % (PKG, os.path.join(GOLDEN, "frontend.npz"), lower)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + lower, PYTHONDONTWRITEBYTECODE="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "workers ok" in out.stdout
