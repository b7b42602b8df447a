"""Writes tests/golden/geometry_offsets.npz: the reference's own compare_lbs_delta.py expressions on a small input.

    python tests/make_golden_geometry.py <path to a checkout of the reference>

A script, not a test.  compare_lbs_delta.py runs a whole job on hard-coded paths when it is imported, so only two pieces
are taken out of it with ``ast`` at generation time: the function ``map_offset_to_color`` and the right-hand side of the
assignment ``offsets = np.sum(...)`` (the weighted offset of a ray), evaluated with ``res`` injected.  Only data is
stored:

  weights  (37, 16) float32, offsets (37, 16, 3) float32     the seeded input (res['weights_on_rays'], res['offset_on_rays'])
  woff     (37, 3)  float32                                  the reference's sum
  color    (37, 3)  float32                                  map_offset_to_color(woff)
  color8   (37, 3)  uint8                                    (color * 255).astype(np.uint8), the tool's quantisation
                                                             of its float32 image

A third of the rays carry offsets large enough to leave the colour map's range on either side."""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'geometry_offsets.npz')
R, S = 37, 16


def _pieces(checkout):
    path = os.path.join(checkout, 'compare_lbs_delta.py')
    with open(path) as f:
        tree = ast.parse(f.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'map_offset_to_color']
    sums = [n.value for n in ast.walk(tree) if isinstance(n, ast.Assign) and len(n.targets) == 1
            and isinstance(n.targets[0], ast.Name) and n.targets[0].id == 'offsets' and isinstance(n.value, ast.Call)]
    assert len(fn) == 1 and len(sums) == 1, path
    return (compile(ast.Module(body=fn, type_ignores=[]), path, 'exec'),
            compile(ast.Expression(body=sums[0]), path, 'eval'))


def inputs():
    rs = np.random.RandomState(41)
    w = rs.uniform(0, 1, (R, S)) ** 4
    w = (w / w.sum(1, keepdims=True) * rs.uniform(0.3, 1.0, (R, 1))).astype(np.float32)
    off = rs.normal(0, 0.012, (R, S, 3))
    off[::3] *= 4.0                                  # beyond +-0.02 on both sides
    off[1] = 0.0                                     # the zero offset: the middle of the map
    return w, off.astype(np.float32)


def main(checkout):
    fn_code, sum_code = _pieces(checkout)
    w, off = inputs()
    ns = {'np': np}
    exec(fn_code, ns)
    woff = eval(sum_code, {'np': np, 'res': {'offset_on_rays': off, 'weights_on_rays': w}})
    color = ns['map_offset_to_color'](woff)
    img = np.zeros(color.shape, np.float32)          # the tool paints into a float32 image, then quantises it
    img[:] = color
    color8 = (img * 255).astype(np.uint8)
    assert woff.dtype == np.float32 and (color8 == 0).any() and (color8 == 255).any()
    np.savez_compressed(OUT, weights=w, offsets=off, woff=woff, color=np.asarray(color), color8=color8)
    print(OUT, os.path.getsize(OUT), 'bytes; color dtype', np.asarray(color).dtype)
    assert os.path.getsize(OUT) <= 100 * 1000


if __name__ == '__main__':
    main(sys.argv[1])
