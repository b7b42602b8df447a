"""Drop-in at the reference's plugin boundary (core/nets/create_network.py:6-15): the reference
loads ``cfg.network_module`` with imp.load_source and calls ``Network()``.  What the reference
brings to that boundary is stored in tests/golden/dropin_reference.json (oracle/make_golden_dropin.py):
its ``configs.cfg`` singleton after the drop-in yaml, the key / shape layout of its own
``Network().state_dict()`` and the groups its ``get_optimizer`` builds over this package's Network.
A ``configs`` module holding that cfg stands in for the reference's package.  Executed in a
subprocess because ``configs`` must be in sys.modules before humannerf_amd.config is imported."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'dropin_reference.json')

SCRIPT = r'''
import imp, json, os, sys, types
sys.dont_write_bytecode = True
ROOT, FIXTURE = %r, %r
sys.path.insert(0, ROOT)
with open(FIXTURE) as f:
    rec = json.load(f)


class Node(dict):
    """attribute-access config node, the interface of the reference's yacs CfgNode"""
    def __init__(self, d):
        super().__init__({k: Node(v) if isinstance(v, dict) else v for k, v in d.items()})

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value


configs = types.ModuleType('configs')
configs.cfg = cfg = Node(rec['cfg'])                 # the reference's singleton, as its train.py / run.py leave it
sys.modules['configs'] = configs
import torch
assert cfg.network_module == 'humannerf_amd.network'
# what create_network() does, with the path resolved against this repo instead of the cwd
mine = imp.load_source(cfg.network_module, os.path.join(ROOT, cfg.network_module.replace('.', '/') + '.py')).Network()
from humannerf_amd import config as hcfg
assert hcfg.cfg is cfg, 'the build must use the reference cfg singleton when it is loaded'
a = {k: tuple(s) for k, s in rec['state_dict']}
b = {k: tuple(v.shape) for k, v in mine.state_dict().items()}
assert a == b, set(a) ^ set(b)
g = torch.Generator().manual_seed(0)
ref_sd = {k: torch.randn(s, generator=g) * 0.01 for k, s in rec['state_dict']}
mine.load_state_dict(ref_sd, strict=True)          # a reference checkpoint loads unchanged
assert mine.deploy_mlps_to_secondary_gpus() is mine
# optimizer routing of the reference works on our parameter names: the groups it built over this Network name
# exactly our parameters, and Adam accepts them in that form
params = dict(mine.named_parameters())
assert [n for _, _, n in rec['optimizer_groups']] == list(params), 'parameter names moved since the fixture was made'
opt = torch.optim.Adam([{'params': [params[n]], 'lr': lr, 'name': gn} for gn, lr, n in rec['optimizer_groups']],
                       lr=cfg.train.lr, betas=(0.9, 0.999))
names = {grp['name'] for grp in opt.param_groups}
assert {'mweight_vol_decoder', 'pose_decoder', 'non_rigid_mlp'} <= names
# late mutation of the shared cfg is what the hot path reads
cfg.perturb = 0.
assert hcfg.cfg.perturb == 0.
print('DROPIN_OK', len(a))
'''


def test_network_is_a_drop_in_for_the_reference_factory():
    r = subprocess.run([sys.executable, '-c', SCRIPT % (ROOT, FIXTURE)], capture_output=True, text=True, timeout=600)
    assert 'DROPIN_OK 55' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
