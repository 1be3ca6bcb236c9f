"""The cases of tests/golden/synthetic_shapes.npz, shared by its generator (tests/golden/make_golden_shapes.py) and the
tests: the configs the cases run with, the fixture reader, and the log of drawing calls a plan stands for."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'synthetic_shapes.npz')
CIRCLE, LINE, FILL_POLY, FILL_CONVEX, ELLIPSE, BLUR, THRESHOLD, RANDU = 1, 2, 3, 4, 5, 6, 7, 8
PRIMITIVES = ['draw_lines', 'draw_polygon', 'draw_multiple_polygons', 'draw_ellipses', 'draw_star', 'draw_checkerboard',
              'draw_stripes', 'draw_cube', 'gaussian_noise']


def small_generation(scale_cube):
    """Blob radii and kernel ranges scaled down to the test frames; the cube's translation range made whole at 96 x 128."""
    g = {'generate_background': {'min_kernel_size': 5, 'max_kernel_size': 20, 'min_rad_ratio': 0.02, 'max_rad_ratio': 0.06},
         'draw_multiple_polygons': {'kernel_boundaries': (3, 9), 'nb_blobs': 100}}
    if scale_cube:
        g['draw_cube'] = {'trans_interval': (0.5, 0.25)}
    return g


def cases():
    """(name, primitive, generation_size, image_size, blur_size, ir_blur_size, scale_cube, keep_canvas)"""
    out = []
    for p in PRIMITIVES:
        out.append(('a_%s' % p, p, (96, 128), (48, 64), 5, 9, True, True))
    for p in ('draw_cube', 'draw_checkerboard', 'draw_stripes', 'draw_lines', 'draw_star'):
        out.append(('b_%s' % p, p, (90, 120), (60, 80), 5, 9, False, False))
    for p in ('draw_polygon', 'draw_multiple_polygons', 'draw_ellipses', 'gaussian_noise'):
        out.append(('c_%s' % p, p, (37, 53), (37, 53), 5, 9, False, False))
    out.append(('d_draw_polygon_default_blur', 'draw_polygon', (96, 128), (48, 64), 21, 51, False, False))
    out.append(('d_draw_ellipses_default_blur', 'draw_ellipses', (96, 128), (48, 64), 21, 51, False, False))
    return out


CASE_NAMES = [c[0] for c in cases()]


def config_of(primitive, gen, img, blur, ir_blur, scale_cube):
    return {'primitives': [primitive], 'generation_size': list(gen), 'image_size': list(img),
            'generation': small_generation(scale_cube),
            'processing': {'blur_size': blur, 'additional_ir_blur': True, 'additional_ir_blur_size': ir_blur},
            'augmentation': {'photometric': {'enable': False}, 'homographic': {'enable': False}}}


def case_config(name):
    for c in cases():
        if c[0] == name:
            return config_of(*c[1:7])
    raise KeyError(name)


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def case(name):
    f = fixture()
    return {k[len('case_%s_' % name):]: v for k, v in f.items() if k.startswith('case_%s_' % name)}


def plan_log(plan, backgrounds):
    """The drawing calls the reference makes for this plan, in the generator's log format: per call the code, the number of
    arguments, the arguments (integer geometry, then the colour).  backgrounds[k] is the background value of the k-th
    get_random_color call; a colour the plan leaves to the device resolves against it."""
    log = []

    def call(code, *args):
        log.extend([float(code), float(len(args))] + [float(a) for a in args])

    def color(spec):
        return spec.a if spec.call < 0 else spec.resolve(backgrounds[spec.call])
    for c in plan.commands:
        kind = c['kind']
        if kind == 'threshold':
            call(THRESHOLD, c['t'])
        elif kind == 'blobs':
            for i, ((x, y, r), (a, b)) in enumerate(zip(c['circles'], c['colors'])):
                call(CIRCLE, x, y, r, b if c['resolve'] and abs(a - backgrounds[c['call0'] + i]) < c['min_contrast'] else a)
        elif kind == 'box_blur':
            call(BLUR, c['k'])
        elif kind == 'line':
            call(LINE, c['p1'][0], c['p1'][1], c['p2'][0], c['p2'][1], c['thickness'], color(c['color']))
        elif kind in ('convex', 'poly'):
            call(FILL_CONVEX if kind == 'convex' else FILL_POLY, *(list(np.asarray(c['points']).reshape(-1)) + [color(c['color'])]))
        elif kind == 'ellipse':
            call(ELLIPSE, c['center'][0], c['center'][1], c['axes'][0], c['axes'][1], c['angle'], color(c['color']))
        elif kind == 'randu':
            call(RANDU)
    return np.array(log, np.float64)


def replay(commands, H, W, fields=(), mean=0.0):
    """The commands of one plan on the CPU through the restatement, on float32 canvases as the kernels hold them: returns
    (canvas, mean).  A colour left to the device resolves against the mean of the last 'mean' command."""
    import shapes_restatement as S
    canvas = np.zeros((H, W), np.float32)
    aux = np.zeros((H, W), np.float32)
    for c in commands:
        kind = c['kind']
        img = aux if c.get('target', 0) else canvas
        if kind == 'threshold':
            canvas[...] = S.threshold(fields[c['field']], c['t'])
        elif kind == 'mean':
            mean = float(np.mean(canvas.astype(np.float64)))
        elif kind == 'blobs':
            if c['base'] is not None:
                img[...] = c['base'].resolve(mean)
            for (x, y, r), (a, b) in zip(c['circles'], c['colors']):
                S.circle(img, (x, y), r, b if c['resolve'] and abs(a - mean) < c['min_contrast'] else a)
        elif kind == 'box_blur':
            img[...] = S.blur(img, c['k']).astype(np.float32)
        elif kind == 'line':
            S.line(img, c['p1'], c['p2'], c['color'].resolve(mean), c['thickness'])
        elif kind == 'convex':
            S.fill_convex_poly(img, c['points'], c['color'].resolve(mean))
        elif kind == 'poly':
            if c.get('copy'):
                mask = S.fill_poly(np.zeros((H, W), np.float32), c['points'], 1.0)
                canvas[mask != 0] = aux[mask != 0]
            else:
                S.fill_poly(img, c['points'], c['color'].resolve(mean))
        elif kind == 'ellipse':
            S.ellipse(img, c['center'], c['axes'], c['angle'], c['color'].resolve(mean))
        else:
            raise ValueError(kind)
    return canvas, mean
