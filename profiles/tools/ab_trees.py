"""Two checkouts of this repository, each with its own built libhnrf.so, against each other on one GPU: do they compute
the same bits, and at the same speed?  For a refactor of host code (profiles/refactor_host_copies.txt).

    python profiles/tools/ab_trees.py bits  PARENT_TREE THIS_TREE OUT_DIR
    python profiles/tools/ab_trees.py speed PARENT_TREE THIS_TREE OUT_DIR [--runs 3] [--budget SECONDS]

bits   per tree, in processes of their own with the tree as working directory: ``bench.py --dump-outputs`` (the arrays
       must be equal one by one), and -- the ``worker`` form of this file -- run_movement, run_tpose,
       run_heads(kind='movement'), run_mesh_render(kind='tpose') and run_compare_lbs_delta on the synthetic subject of
       tests/golden at its own size, with the multi-head fixture weights: both trees must write the same file names and,
       by ``cmp``, the same bytes in every file.
speed  ``--runs`` times, the trees taking turns: the rates of ``bench.py --full`` (headline, lean_outputs, other_mode,
       culled, terminated, frame_loop, train), run_movement's ms per frame of movement_loop.py and the all-heads frame of
       time_multihead.py --step frame.  Prints the range per tree and value, and whether the ranges overlap.  No round
       is begun that would not end inside ``--budget``, going by the rounds before it.
Every child runs under a time limit; the first one that fails ends the run.  Reads nothing outside the two trees."""
import json
import os
import re
import shutil
import subprocess
import sys
import time

LABELS = ('parent', 'this')


def child(tree, argv, limit, log=None):
    """One process with ``tree`` as its working directory and first import path; returns its stdout."""
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop('HNRF_LIB_PATH', None)
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable] + argv, cwd=tree, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if log:
        with open(log, 'w') as f:
            f.write(p.stdout)
    if p.returncode != 0:
        sys.exit('ab_trees: %s in %s ended with %d; nothing more is started\n%s' % (argv, tree, p.returncode, p.stdout[-3000:]))
    return p.stdout


def worker(out, subject_dir):
    """The five loops in the tree that is the working directory, on the subject in ``subject_dir``, into ``out``."""
    sys.path.insert(0, os.getcwd())
    sys.path.insert(1, os.path.join(os.getcwd(), 'tests'))
    import torch
    import multihead_cases as mc
    from humannerf_amd import dataset, run
    from humannerf_amd.config import cfg
    from humannerf_amd.network import Network
    from humannerf_amd.seeded import default_shapes, seeded_state
    dev = torch.device('cuda:0')
    state = seeded_state(default_shapes(), seed=0)

    def network(state):
        net = Network()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
        return net.to(dev).eval()

    net = network(state)
    subj = dataset.Subject(subject_dir)
    cfg.N_samples, cfg.perturb, cfg.chunk, cfg.bgcolor = 64, 0., 32768, [255., 255., 255.]
    cfg.amd.diagnostics, cfg.amd.video, cfg.amd.maps = False, 'mjpeg', []
    run.run_movement(net, subj, logdir=os.path.join(out, 'movement'), metrics=['psnr'])
    run.run_tpose(net, subj, total_frames=3, image_size=64, logdir=os.path.join(out, 'tpose'))
    run.run_mesh_render(net, subj, kind='tpose', resolution=64, total_frames=3, image_size=(64, 48),
                        logdir=os.path.join(out, 'mesh_tpose'))
    run.run_compare_lbs_delta(net, subj, logdir=os.path.join(out, 'cmp'))
    cfg.amd.video = 'none'
    cfg.canonical_mlp.multihead = {'enable': True, 'head_depth': 1}
    cfg.multihead = {'head_num': 3, 'split': 'view'}
    heads = network(mc.multihead_state(state, 3))
    run.run_heads(heads, subj, kind='movement', logdir=os.path.join(out, 'heads'), metrics=['psnr'])
    torch.cuda.synchronize()
    print('cfg behind the loops:', {k: cfg.get(k) for k in ('perturb', 'ignore_non_rigid_motions', 'show_truth')},
          dict(cfg.amd))


def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def bits(trees, out):
    import numpy as np
    for label, tree in zip(LABELS, trees):
        os.makedirs(os.path.join(out, label), exist_ok=True)
        child(tree, ['bench.py', '--gpus', '1', '--steps', '2', '--warmup', '1', '--main-only', '--dump-outputs',
                     os.path.join(out, label, 'bench')], 300, os.path.join(out, label, 'bench.log'))
        # the tree's own fixture at one path for both: MetricsWriter heads its files with the subject's path
        subject = os.path.join(out, 'subject')
        shutil.rmtree(subject, ignore_errors=True)
        shutil.copytree(os.path.join(tree, 'tests', 'golden', 'subject_synth'), subject)
        log = child(tree, [os.path.abspath(__file__), 'worker', os.path.join(out, label, 'runs'), subject], 420,
                    os.path.join(out, label, 'runs.log'))
        print(label, log.strip().splitlines()[-1])
    bad = 0
    a, b = (os.path.join(out, label) for label in LABELS)
    names = [files_under(os.path.join(r, 'bench')) for r in (a, b)]
    assert names[0] == names[1] and names[0], names
    for n in names[0]:
        x, y = (np.load(os.path.join(r, 'bench', n)) for r in (a, b))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        bad += not same
        print('bench.py --dump-outputs  %-32s %-18s %s' % (n, x.shape, 'equal' if same else 'DIFFERENT'))
    for r in (a, b):
        shutil.rmtree(os.path.join(r, 'bench'))             # (48 MB per tree)
    names = [files_under(os.path.join(r, 'runs')) for r in (a, b)]
    if names[0] != names[1]:
        bad += 1
        print('file names DIFFER:', sorted(set(names[0]) ^ set(names[1])))
    kinds = {}
    for n in names[0]:
        if n in names[1]:
            same = subprocess.run(['cmp', '-s', os.path.join(a, 'runs', n), os.path.join(b, 'runs', n)]).returncode == 0
            bad += not same
            k = kinds.setdefault(os.path.splitext(n)[1], [0, 0])
            k[0] += 1
            k[1] += same
            if not same:
                print('DIFFERENT bytes:', n)
    print('run loops: %d files in each tree; cmp equal / files by suffix: %s' %
          (len(names[0]), ', '.join('%s %d/%d' % (s, k[1], k[0]) for s, k in sorted(kinds.items()))))
    print('bits: %s' % ('SAME' if not bad else '%d DIFFERENCES' % bad))
    return bad


def leaves(line):
    d = json.loads(line)
    got = {'headline rays/s': d['value']}
    for key, field in (('lean_outputs', 'rays_per_s_per_gpu'), ('other_mode', 'rays_per_s_per_gpu'),
                       ('culled', 'rays_per_s_per_gpu'), ('terminated', 'rays_per_s_per_gpu'),
                       ('frame_loop', 'frames_per_s_per_gpu'), ('train', 'iters_per_s')):
        if key in d:
            got['%s %s' % (key, field)] = d[key][field]
    return got


def speed(trees, out, runs, budget):
    os.makedirs(out, exist_ok=True)
    seen = {label: {} for label in LABELS}
    t0 = time.time()
    for r in range(runs):
        if r and time.time() - t0 + (time.time() - t0) / r > budget:        # (a round would not end inside the budget)
            print('stopped after %d of %d rounds: %.0f s of the %.0f s budget used' % (r, runs, time.time() - t0, budget))
            break
        for label, tree in zip(LABELS, trees):
            tag = os.path.join(out, '%s_%d' % (label, r))
            got = leaves(child(tree, ['bench.py', '--gpus', '1', '--steps', '5', '--warmup', '2', '--full',
                                      '--no-cpu-baseline'], 400, tag + '_bench.log').strip().splitlines()[-1])
            text = child(tree, ['profiles/tools/movement_loop.py', '12'], 300, tag + '_movement.log')
            got['movement_loop run_movement ms/frame (lower is better)'] = float(
                re.search(r'run_movement ([\d.]+) ms per frame', text).group(1))
            text = child(tree, ['profiles/tools/time_multihead.py', '--step', 'frame', '--iters', '10'], 300,
                         tag + '_multihead.log')
            frame = json.loads([l for l in text.splitlines() if l.startswith('{')][-1])
            for k, v in sorted(flat(frame).items()):
                if k.endswith('all_heads.median'):
                    got['time_multihead %s ms (lower is better)' % k] = v
            for k, v in got.items():
                seen[label].setdefault(k, []).append(v)
            print(label, r, json.dumps(got), flush=True)
            with open(os.path.join(out, 'speed.json'), 'w') as f:
                json.dump(seen, f, indent=1)
    for k in seen['parent']:
        p, t = seen['parent'][k], seen['this'].get(k, [])
        verdict = 'overlap' if t and min(t) <= max(p) and max(t) >= min(p) else 'APART'
        print('%-62s parent %s .. %s   this %s .. %s   %s' % (k, min(p), max(p), min(t), max(t), verdict))


def flat(d, prefix=''):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(flat(v, prefix + k + '.'))
        elif isinstance(v, (int, float)) and not isinstance(v, bool):
            out[prefix + k] = v
    return out


if __name__ == '__main__':
    if sys.argv[1] == 'worker':
        worker(sys.argv[2], sys.argv[3])
        sys.exit(0)
    what, trees, out = sys.argv[1], [os.path.abspath(p) for p in sys.argv[2:4]], os.path.abspath(sys.argv[4])
    if what == 'bits':
        sys.exit(1 if bits(trees, out) else 0)
    option = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    speed(trees, out, option('--runs', 3), option('--budget', 3600.))
