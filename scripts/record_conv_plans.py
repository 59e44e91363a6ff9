"""Records which kernel the convolution launch rule gives every row of a shape table, by launching: tests/golden/conv_plans.json.

    python scripts/record_conv_plans.py [--out tests/golden/conv_plans.json] [--only GROUP]

Run it against the library whose rule is to be pinned (YOLO2_LIB_PATH selects another build; YOLO2_LIB_COMMIT names the commit that build came from
for the file header, which otherwise takes the checkout's HEAD).  Per row: one call of the row's entry point, then
yolo2_debug_last_conv_plan, yolo2_last_bn_part_rows (statistics-producing entry points only: the others leave the previous launch's value) and, for
dgrad_bn, *pending; next to them the library's yolo2_conv2d_workspace_bytes and yolo2_conv2d_dgrad_bn_fuses for the shape.  Rows of at most 2^20
output elements run on operands from numpy.random.RandomState(row index) and store yolo2_crc32c of the output buffer, unless the launch was K-sliced
(plan word split == 1: its slices meet in f32 atomics); larger rows run on zeros.

The environment knobs are read once per process, so every group of rows -- the default environment, then one group per knob setting -- runs in a
fresh child process, one after another, each under its own time limit; the first non-zero status ends the recording.

tests/test_conv_route_cpu.py reproduces every row with ops.conv_route; tests/test_conv_route_gpu.py launches the default-environment rows again."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WS_FLOATS = 1024 + 256 * 256 * 128          # engine.Engine.conv_ws
CRC_MAX_ELEMS = 1 << 20
# name, H (= W at 416), Cin, Cout (None: the head), ksize, bn -- tests/test_bench_shapes_gpu.py LAYERS
LAYERS = [
    ('conv0', 416, 3, 32, 3, True), ('conv1', 208, 32, 64, 3, True), ('conv2_4', 104, 64, 128, 3, True),
    ('conv3', 104, 128, 64, 1, True), ('conv5_7', 52, 128, 256, 3, True), ('conv6', 52, 256, 128, 1, True),
    ('conv8_10_12', 26, 256, 512, 3, True), ('conv9_11', 26, 512, 256, 1, True), ('conv13_15_17', 13, 512, 1024, 3, True),
    ('conv14_16', 13, 1024, 512, 1, True), ('conv18_19', 13, 1024, 1024, 3, True), ('conv20', 13, 3072, 1024, 3, True),
    ('conv_out', 13, 1024, None, 1, False),
]
# tests/test_kernels_gpu.py: CONV_SHAPES, the K-sliced / stream-K list, the statistics list, the persistent-kernel lists, TAP_SHAPES, the dgrad_bn list
CONV_SHAPES = [(2, 13, 13, 16, 40, 3), (1, 26, 20, 3, 32, 3), (2, 33, 70, 3, 32, 3), (1, 64, 96, 3, 32, 3), (2, 13, 13, 64, 125, 1), (2, 26, 26, 64, 160, 3),
               (1, 8, 8, 24, 64, 3), (3, 5, 7, 136, 72, 3), (1, 13, 13, 192, 128, 3), (2, 12, 20, 32, 64, 3), (1, 7, 9, 32, 64, 3), (3, 40, 33, 32, 64, 3),
               (2, 9, 11, 320, 200, 3), (2, 12, 20, 64, 128, 3), (2, 12, 20, 64, 32, 3), (2, 12, 20, 128, 64, 3), (1, 7, 9, 64, 128, 3), (3, 40, 33, 64, 128, 3)]
KSLICED_SHAPES = [(2, 13, 13, 512, 256, 3), (1, 13, 13, 1024, 125, 1), (2, 26, 26, 256, 136, 3), (8, 13, 13, 1024, 500, 3), (16, 13, 13, 3072, 1000, 1)]
BN_SHAPES = [(2, 26, 26, 64, 160, 3), (1, 64, 96, 3, 32, 3), (2, 13, 13, 512, 256, 3), (8, 13, 13, 1024, 504, 3), (3, 20, 20, 32, 64, 3), (2, 13, 13, 128, 256, 1),
             (1, 65, 64, 72, 136, 3)]
PERSISTENT_SHAPES = [(3, (3, 40, 33, 32, 64, 3)), (1, (4, 40, 33, 32, 64, 3)), (2, (1, 5, 300, 32, 64, 3)), (0, (1, 3, 500, 32, 64, 3)),
                     (3, (3, 40, 33, 64, 128, 3)), (5, (2, 31, 16, 64, 128, 3)), (0, (2, 26, 27, 64, 128, 3)), (2, (1, 6, 200, 64, 128, 3)),
                     (0, (1, 4, 320, 64, 128, 3))]
TAP_SHAPES = [(16, 13, 13, 512, 1024), (16, 26, 26, 256, 512), (9, 52, 52, 128, 256), (8, 13, 13, 1024, 504), (16, 26, 26, 256, 136), (16, 55, 55, 128, 128),
              (16, 13, 13, 3072, 1024), (16, 13, 13, 1024, 512), (16, 26, 26, 512, 256), (3, 5, 7, 64, 72), (2, 19, 19, 128, 200), (1, 27, 28, 192, 128),
              (5, 10, 10, 320, 264)]
# (B, H, W, filters of the consumer = Cp, channels = Nf, k)
DGRAD_BN_SHAPES = [(2, 26, 26, 160, 64, 3), (16, 13, 13, 1024, 512, 3), (8, 13, 13, 1024, 504, 3), (4, 52, 52, 256, 128, 3), (2, 26, 26, 512, 256, 1),
                   (3, 20, 20, 64, 32, 3), (2, 13, 13, 512, 256, 3), (2, 104, 104, 64, 128, 1), (4, 52, 52, 128, 256, 1), (3, 53, 55, 64, 384, 1)]
KNOBS = [('YOLO2_C32', '0'), ('YOLO2_C64', '0'), ('YOLO2_D1', '0'), ('YOLO2_FIRST_DIRECT', '0'), ('YOLO2_IGEMM_TAP', '0'), ('YOLO2_IGEMM_TAP', '3'),
         ('YOLO2_IGEMM_STREAM', '0')]


def pad8(c):
    return (c + 7) // 8 * 8


def row(entry, dtype, B, H, W, Cp, Nf, k, ldp=None, ldo=None, ws=WS_FLOATS, det=0, wgs=0, tag=''):
    return dict(entry=entry, dtype=dtype, B=B, H=H, W=W, Cp=Cp, ldp=ldp or Cp, Nf=Nf, ldo=ldo or Nf, k=k, ws_floats=ws, det=det, wgs=wgs, tag=tag)


def layer_rows(name, B, S, cin, cout, k, bn, fwd=('bn', 'bias_leaky'), dgr=('ws', 'dgrad_bn'), **kw):
    """The rows of one Darknet-19 layer at batch B, S x S pixels: forward as the engine calls it in training and inference, data gradient plain and
    with the producer's BN-backward sums."""
    ldx, ldy = pad8(cin), pad8(cout)
    out = []
    for e in fwd:
        if e == 'bn' and not bn:
            e = 'ws_bias'
        if e == 'bias_leaky' and not bn:
            continue
        out.append(row(e, 'bf16', B, S, S, ldx, cout, k, ldo=ldy, tag='%s fwd' % name, **kw))
    if name != 'conv0':
        for e in dgr:
            out.append(row(e, 'bf16', B, S, S, ldy, cin, k, ldo=ldx, tag='%s dgrad' % name, **kw))
    return out


def default_rows():
    rows = []
    for B, head in ((16, 125), (8, 425)):                                   # the benchmark shapes
        for name, S, cin, cout, k, bn in LAYERS:
            rows += layer_rows(name, B, S, cin, cout or head, k, bn, fwd=('bn', 'bias_leaky') if B == 16 else ('bn',))
    for size in (320, 608):                                                 # the multi-scale sizes
        for name, S, cin, cout, k, bn in LAYERS:
            rows += layer_rows(name, 8, S * size // 416, cin, cout or 425, k, bn, fwd=('bn',), dgr=('dgrad_bn',))
    for B in (4, 32):
        for name, S, cin, cout, k, bn in LAYERS:
            if S <= 26:
                rows += layer_rows(name, B, S, cin, cout or 125, k, bn, fwd=('bn',), dgr=('dgrad_bn',))
    for dt in ('f32', 'bf16'):                                              # small shapes, as tests/test_kernels_gpu.py calls them
        for B, H, W, cin, cout, k in CONV_SHAPES:
            rows.append(row('conv2d_bias' if k == 1 else 'conv2d', dt, B, H, W, pad8(cin), cout, k, ldo=pad8(cout), ws=0, tag='small fwd'))
            rows.append(row('conv2d', dt, B, H, W, pad8(cout), cin, k, ldo=pad8(cin), ws=0, tag='small dgrad'))
        for B, H, W, cin, cout, k in KSLICED_SHAPES:
            rows.append(row('ws_bias', dt, B, H, W, cin, cout, k, ldo=pad8(cout), ws=max(B * H * W * cout + 64, 1024 + 256 * 128 * 128), tag='ksliced'))
        for B, H, W, cin, cout, k in BN_SHAPES:
            rows.append(row('bn', dt, B, H, W, pad8(cin), cout, k, tag='bn'))
        for B, H, W, cp, nf, k in DGRAD_BN_SHAPES:
            rows.append(row('dgrad_bn', dt, B, H, W, cp, nf, k, tag='dgrad_bn'))
    for wgs, (B, H, W, cin, cout, k) in PERSISTENT_SHAPES:
        for e in ('ws', 'bias_leaky', 'bn'):
            rows.append(row(e, 'bf16', B, H, W, cin, cout, k, wgs=wgs, tag='persistent'))
    for wgs, (B, H, W, cin, cout, k) in ((3, (3, 40, 33, 64, 32, 3)), (0, (2, 12, 20, 128, 64, 3)), (2, (2, 12, 20, 64, 32, 3))):
        for e in ('ws', 'bias_leaky'):      # the plain-store forms of conv_c64.hip step aside for an epilogue
            rows.append(row(e, 'bf16', B, H, W, cin, cout, k, wgs=wgs, tag='persistent'))
    for B, H, W, cin, cout in TAP_SHAPES:
        for e in ('ws', 'dgrad_bn'):
            if e == 'ws' or cout % 8 == 0:
                rows.append(row(e, 'bf16', B, H, W, cin, cout, 3, ldo=pad8(cout), tag='tap'))
    # every generic variant, both dtypes and kernel sizes (v4 / v8: channels of a 64- / 128-byte K row)
    for dt, v in (('f32', 4), ('bf16', 8)):
        v4, v8 = 4 * v, 8 * v
        for k in (1, 3):
            for e in ('ws', 'dgrad_bn'):
                for nf in (32, 64):
                    rows.append(row(e, dt, 2, 13, 13, 3 * v4, nf, k, tag='narrow'))                  # 64-byte rows
                    rows.append(row(e, dt, 2, 13, 13, 3 * v, nf, k, tag='narrow channel tail'))
                    rows.append(row(e, dt, 2, 13, 13, 3 * v8, nf, k, tag='narrow 128-byte rows'))    # (3x3: the 2-stage ring)
                rows.append(row(e, dt, 2, 13, 13, 3 * v4, 128, k, tag='8 waves 64-byte rows'))
                rows.append(row(e, dt, 2, 13, 13, 3 * v, 128, k, tag='8 waves channel tail'))
                rows.append(row(e, dt, 2, 13, 13, v8, 128, k, tag='wide'))
                rows.append(row(e, dt, 2, 104, 104, 3 * v8, 256, k, tag='2-stage'))
                kc = 16 * v8 if k == 3 else 128 * v4                                                  # >= 128 K tiles of 64 bytes
                rows.append(row(e, dt, 1, 13, 13, kc, 128, k, tag='k-sliced'))
                rows.append(row(e, dt, 1, 13, 13, kc + v, 128, k, tag='k-sliced channel tail'))
                rows.append(row(e, dt, 16, 13, 13, 48 * v8, 1000, k, tag='stream-K 128x128'))         # (bf16 3x3: the ping-pong kernel)
                rows.append(row(e, dt, 16, 13, 13, (16 if k == 3 else 128) * v8, 1024, k, tag='256x128'))
                rows.append(row(e, dt, 1, 13, 64, (16 if k == 3 else 128) * v8, 2048, k, tag='256x128, image wider than 55'))
    rows.append(row('ws_bias', 'bf16', 16, 13, 13, 1024, 125, 1, ldo=160, tag='concat-slice stride: no 16-byte stores'))
    rows.append(row('ws', 'bf16', 2, 26, 26, 256, 120, 3, ldo=512, tag='concat-slice stride: no 16-byte stores'))
    rows.append(row('ws', 'bf16', 16, 13, 13, 1024, 1024, 3, ldo=1280, tag='concat slice'))
    for name, S, cin, cout, k, bn in LAYERS:
        if S <= 26:
            for kw in (dict(ws=4096), dict(det=1)):            # workspace too small: no stream-K, no K slicing; deterministic: no K slicing
                rows += layer_rows(name, 16, S, cin, cout or 125, k, bn, fwd=('bn',), dgr=('dgrad_bn',), **kw)
    for kw in (dict(ws=4096), dict(det=1)):
        rows.append(row('ws_bias', 'bf16', 2, 13, 13, 512, 256, 3, tag='ksliced', **kw))
        rows.append(row('ws_bias', 'f32', 1, 13, 13, 2048, 128, 1, tag='ksliced', **kw))
    return rows


def knob_rows(name, value):
    want = {
        'YOLO2_C32': lambda n, S, cin, k: n == 'conv1',
        'YOLO2_C64': lambda n, S, cin, k: n in ('conv1', 'conv2_4'),
        'YOLO2_D1': lambda n, S, cin, k: n in ('conv3', 'conv6'),
        'YOLO2_FIRST_DIRECT': lambda n, S, cin, k: n == 'conv0',
        'YOLO2_IGEMM_TAP': lambda n, S, cin, k: k == 3 and S <= 52,
        'YOLO2_IGEMM_STREAM': lambda n, S, cin, k: S <= 26,
    }[name]
    rows = []
    for B, head in ((16, 125), (8, 425)):
        for n, S, cin, cout, k, bn in LAYERS:
            if want(n, S, cin, k):
                rows += layer_rows(n, B, S, cin, cout or head, k, bn, fwd=('bn',), dgr=('ws', 'dgrad_bn') if B == 16 else ('dgrad_bn',))
    if name == 'YOLO2_IGEMM_TAP':
        for B, H, W, cin, cout in TAP_SHAPES[9:]:
            rows.append(row('ws', 'bf16', B, H, W, cin, cout, 3, ldo=pad8(cout), tag='tap'))
    return rows


def run_rows(rows, first_index):
    import ctypes
    import numpy as np
    import torch
    from yolo_tf_amd import ops, _lib
    lib = _lib.load()
    out = []
    for i, r in enumerate(rows):
        idx = first_index + i
        T = torch.bfloat16 if r['dtype'] == 'bf16' else torch.float32
        B, H, W, Cp, ldp, Nf, ldo, k = (r[x] for x in ('B', 'H', 'W', 'Cp', 'ldp', 'Nf', 'ldo', 'k'))
        M = B * H * W
        seeded = M * ldo <= CRC_MAX_ELEMS
        rng = np.random.RandomState(idx)

        def t(n, scale=1.0, dtype=T, pos=False):
            if not seeded:
                return torch.zeros(n, dtype=dtype, device='cuda')
            a = (rng.rand(n) + 0.5 if pos else rng.randn(n) * scale).astype(np.float32)
            return torch.from_numpy(a).to('cuda').to(dtype)

        P, F = t(M * ldp), t(Nf * k * k * Cp, 1.0 / np.sqrt(k * k * Cp))
        O = torch.zeros(M * ldo, dtype=T, device='cuda')
        ws = torch.full((r['ws_floats'],), 3.0, dtype=torch.float32, device='cuda') if r['ws_floats'] else None
        e = r['entry']
        pending = None
        ops.set_deterministic(r['det'])
        if r['wgs']:
            ops.set_stream_workgroups(r['wgs'])
        try:
            if e in ('conv2d', 'conv2d_bias'):
                ops.conv2d(P, F, t(Nf, dtype=torch.float32) if e == 'conv2d_bias' else None, O, B, H, W, Cp, ldp, Nf, ldo, k)
            elif e in ('ws', 'ws_bias'):
                bias = t(Nf, dtype=torch.float32) if e == 'ws_bias' else None
                if ws is None:
                    _lib.call('yolo2_conv2d_ws', P.data_ptr(), F.data_ptr(), _lib.ptr(bias), O.data_ptr(), None, 0, B, H, W, Cp, ldp, Nf, ldo, k, _lib.dtype_code(T), ops._stream())
                else:
                    ops.conv2d_ws(P, F, bias, O, ws, B, H, W, Cp, ldp, Nf, ldo, k)
            elif e == 'bias_leaky':
                ws_ = ws if ws is not None else torch.zeros(0, dtype=torch.float32, device='cuda')
                ops.conv2d_bias_leaky(P, F, t(Nf, dtype=torch.float32), O, ws_, B, H, W, Cp, ldp, Nf, ldo, k, 0.1)
            elif e == 'bn':
                part = torch.zeros(2 * 256 * Nf, dtype=torch.float32, device='cuda')
                ws_ = ws if ws is not None else torch.zeros(0, dtype=torch.float32, device='cuda')
                ops.conv2d_bn(P, F, O, ws_, B, H, W, Cp, ldp, Nf, ldo, k, t(Nf, 0.1, dtype=torch.float32), part)
            elif e == 'dgrad_bn':
                part = torch.zeros(2 * 256 * Nf, dtype=torch.float32, device='cuda')
                ws_ = ws if ws is not None else torch.zeros(0, dtype=torch.float32, device='cuda')
                f32 = torch.float32
                Y, mean, var, gamma, beta = t(M * Nf), t(Nf, 0.1, f32), t(Nf, dtype=f32, pos=True), t(Nf, dtype=f32, pos=True), t(Nf, 0.1, f32)
                dg, db = torch.zeros(Nf, device='cuda'), torch.zeros(Nf, device='cuda')
                red = torch.zeros(max(1, int(_lib.query('yolo2_bn_workspace_bytes', Nf)) // 8), dtype=torch.float64, device='cuda')
                pending = int(ops.conv2d_dgrad_bn(P, F, O, ws_, B, H, W, Cp, ldp, Nf, ldo, k, Y, mean, var, gamma, beta, dg, db, part, red, 1e-5, 0.1))
            else:
                raise ValueError(e)
            plan = [ops.last_conv_plan()[key] for key in ops.CONV_PLAN_KEYS]
            rows_used = ops.last_bn_part_rows() if e in ('bn', 'dgrad_bn') else None
            torch.cuda.synchronize()
        finally:
            ops.set_deterministic(0)
            if r['wgs']:
                ops.set_stream_workgroups(0)
        crc = None
        if seeded and (plan[5] & 0xff) != 1:
            raw = O.view(torch.uint8).cpu().numpy().tobytes()
            crc = int(lib.yolo2_crc32c(ctypes.c_char_p(raw), len(raw), 0))
        res = dict(r)
        dt_code = _lib.dtype_code(T)
        res.update(index=idx, plan=plan, rows=rows_used, pending=pending, crc=crc,
                   ws_bytes_query=int(lib.yolo2_conv2d_workspace_bytes(B, H, W, Cp, Nf, k, dt_code)),
                   fuses_query=int(lib.yolo2_conv2d_dgrad_bn_fuses(B, H, W, Nf, k, dt_code)))
        out.append(res)
        del P, F, O, ws
    ops.check_async_errors()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return out, cus


def groups():
    out = [('default', {}, default_rows())]
    for name, value in KNOBS:
        out.append(('%s=%s' % (name, value), {name: value}, knob_rows(name, value)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'conv_plans.json'))
    ap.add_argument('--only', default=None, help='record one group only (its name, e.g. default or YOLO2_C32=0)')
    ap.add_argument('--list', action='store_true', help='print the row counts and exit (no device)')
    ap.add_argument('--child', type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--first-index', type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    gs = groups()
    if args.list:
        for name, env, rows in gs:
            print('%-24s %d rows' % (name, len(rows)))
        return 0
    if args.child is not None:
        name, env, rows = gs[args.child]
        res, cus = run_rows(rows, args.first_index)
        for r in res:
            r['env'] = env
        json.dump(dict(cus=cus, rows=res), open(args.out, 'w'))
        return 0
    commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True).stdout.strip() or 'unknown'
    lib_note = os.environ.get('YOLO2_LIB_COMMIT')      # a library built from another commit (scripts/build_baseline.sh) says so itself
    doc = dict(library_commit=lib_note or commit, cus=None, ws_floats=WS_FLOATS, plan_keys=['BM', 'BN', 'waves', 'chunks', 'stages', 'split', 'grid_x', 'grid_y'], rows=[])
    first = 0
    for gi, (name, env, rows) in enumerate(gs):
        if args.only and name != args.only:
            first += len(rows)
            continue
        part = args.out + '.part%d' % gi
        child_env = dict(os.environ)
        child_env.update(env)
        print('group %s: %d rows' % (name, len(rows)), flush=True)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(gi), '--first-index', str(first), '--out', part], env=child_env,
                            timeout=240).returncode
        if rc != 0:
            print('group %s ended with status %d: recording stopped' % (name, rc), file=sys.stderr)
            return rc or 1
        got = json.load(open(part))
        os.remove(part)
        doc['cus'] = got['cus']
        doc['rows'] += got['rows']
        first += len(rows)
    with open(args.out, 'w') as f:
        f.write('{\n')
        for key in ('library_commit', 'cus', 'ws_floats', 'plan_keys'):
            f.write(' %s: %s,\n' % (json.dumps(key), json.dumps(doc[key])))
        f.write(' "rows": [\n')
        f.write(',\n'.join('  ' + json.dumps(r, sort_keys=True, separators=(',', ':')) for r in doc['rows']))
        f.write('\n ]\n}\n')
    print('wrote %s: %d rows' % (args.out, len(doc['rows'])))
    return 0


if __name__ == '__main__':
    sys.exit(main())
