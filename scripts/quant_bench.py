"""int8 inference against bf16 on the MI355X, in ONE process (profiles/quant_int8.md):

  * per layer of darknet-20 at 416 x 416, batches 16 and 256: yolo2_conv2d_i8 (int8 output, leaky) against yolo2_conv2d_bias_leaky (bf16),
    alternating the two, each timed over enough launches to fill ~50 ms;
  * DetectSession.detect end to end, int8 against bf16, alternating, at batches 64 and 256;
  * calibration cost per batch;
  * relative L2 of the int8 logits against the bf16 logits, seeded weights.

usage: python scripts/quant_bench.py [--out FILE] [--layers-only | --detect-only] [--batches 16,256] [--detect-batches 64,256]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from yolo_tf_amd import ops

LAYERS = [  # name, H, Cin, Cout, k, layers of this shape in the network (conv0 stays bf16)
    ('conv1', 208, 32, 64, 3, 1), ('conv2', 104, 64, 128, 3, 2), ('conv3', 104, 128, 64, 1, 1), ('conv5', 52, 128, 256, 3, 2),
    ('conv6', 52, 256, 128, 1, 1), ('conv8', 26, 256, 512, 3, 3), ('conv9', 26, 512, 256, 1, 2), ('conv13', 13, 512, 1024, 3, 3),
    ('conv14', 13, 1024, 512, 1, 2), ('conv18', 13, 1024, 1024, 3, 2), ('conv20', 13, 3072, 1024, 3, 1), ('convout', 13, 1024, 125, 1, 1)]


def time_us(fn, target_ms=50.0):
    """Mean device time of one call in microseconds: warm-up, a pilot to size the window, then device events around the window."""
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    n = int(max(5, min(2000, target_ms / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def layers(batches):
    rows = []
    for B in batches:
        need = max(ops.workspace_bytes('conv2d', B, H, H, cin, cout, k, ops.dtype_code(torch.bfloat16)) for _, H, cin, cout, k, _ in LAYERS)
        ws = torch.zeros(need // 4 + 1024, dtype=torch.float32, device='cuda')
        for name, H, cin, cout, k, count in LAYERS:
            M = B * H * H
            ldo = ops.pad8(cout)
            x = torch.randn(M * cin, device='cuda').to(torch.bfloat16)
            f = (torch.randn(cout * k * k * cin, device='cuda') * 0.05).to(torch.bfloat16)
            bias = torch.zeros(cout, dtype=torch.float32, device='cuda')
            y = torch.zeros(M * ldo, dtype=torch.bfloat16, device='cuda')
            xq = torch.randint(-127, 128, (M * cin,), dtype=torch.int8, device='cuda')
            fq = torch.randint(-127, 128, (cout * k * k * cin,), dtype=torch.int8, device='cuda')
            mult = torch.full((cout,), 1e-5, dtype=torch.float32, device='cuda')
            yq = torch.zeros(M * ldo, dtype=torch.int8, device='cuda')
            bf = lambda: ops.conv2d_bias_leaky(x, f, bias, y, ws, B, H, H, cin, cin, cout, ldo, k, 0.1)      # noqa: E731
            i8 = lambda: ops.conv2d_i8(xq, fq, mult, bias, yq, B, H, H, cin, cin, cout, ldo, k, 0.1, 1.0, ops.I8_OUT_I8)      # noqa: E731
            t = {'bf16': [], 'int8': []}
            for _ in range(2):              # alternate the two
                t['bf16'].append(time_us(bf))
                t['int8'].append(time_us(i8))
            flops = 2.0 * M * cout * k * k * cin
            row = dict(batch=B, layer=name, count=count, bf16_us=min(t['bf16']), int8_us=min(t['int8']), bf16_all=t['bf16'], int8_all=t['int8'],
                       bf16_tflops=flops / min(t['bf16']) * 1e-6, int8_tops=flops / min(t['int8']) * 1e-6)
            rows.append(row)
            print('B %3d %-8s bf16 %9.1f us %7.1f TFLOP/s | int8 %9.1f us %7.1f TOP/s | int8/bf16 time %.2f' % (
                B, name, row['bf16_us'], row['bf16_tflops'], row['int8_us'], row['int8_tops'], row['int8_us'] / row['bf16_us']), flush=True)
            del x, f, y, xq, fq, yq
        tot_b = sum(r['bf16_us'] * r['count'] for r in rows if r['batch'] == B)
        tot_i = sum(r['int8_us'] * r['count'] for r in rows if r['batch'] == B)
        print('B %3d conv1..head, weighted by layer count: bf16 %.1f us, int8 %.1f us, int8/bf16 %.2f' % (B, tot_b, tot_i, tot_i / tot_b), flush=True)
    return rows


def detect(batches, size=416):
    from bench import make_builder
    from yolo_tf_amd import quant
    from yolo_tf_amd.session import DetectSession
    rows = []
    basedir = tempfile.mkdtemp(prefix='quant_bench_')
    for B in batches:
        b, _ = make_builder('darknet', 20, size, False, basedir)
        b8, _ = make_builder('darknet', 20, size, False, basedir)
        sess = DetectSession(b, B, dtype='bf16', seed=0)
        images = torch.from_numpy(np.random.RandomState(1).uniform(0, 255, (B, size, size, 3)).astype(np.float32)).cuda()
        cal = quant.Calibrator(sess)
        cal.observe(images)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            cal.observe(images)
        torch.cuda.synchronize()
        cal_ms = (time.perf_counter() - t0) / 3 * 1e3
        calibration = cal.finish()
        del cal
        torch.cuda.empty_cache()
        sess8 = DetectSession(b8, B, dtype='int8', seed=0, calibration=calibration)
        sess8.engine.set_variables(sess.engine.get_variables())
        t = {'bf16': [], 'int8': []}
        for _ in range(2):
            t['bf16'].append(time_us(lambda: sess.detect(images), 300.0) / 1e3)
            t['int8'].append(time_us(lambda: sess8.detect(images), 300.0) / 1e3)
        sess.run(images, check_numerics=False)
        sess8.run(images, check_numerics=False)
        out = sess.engine.output()
        n = B * out.h * out.w * sess.engine.act[out][1]
        ref = sess.engine.act[out][0][:n].float().cpu().numpy().astype(np.float64)
        got = sess8.engine.act[sess8.engine.output()][0][:n].float().cpu().numpy().astype(np.float64)
        rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        act8 = sum(r.numel() * r.element_size() for r in sess8.engine._roots.values())
        row = dict(batch=B, bf16_ms=min(t['bf16']), int8_ms=min(t['int8']), bf16_all=t['bf16'], int8_all=t['int8'], calibrate_ms_per_batch=cal_ms,
                   logits_rel_l2_int8_vs_bf16=rel, int8_activation_bytes=act8)
        rows.append(row)
        print('detect B %3d: bf16 %.3f ms, int8 %.3f ms, int8/bf16 %.2f; calibration %.1f ms per batch; logits rel L2 int8 vs bf16 %.4f' % (
            B, row['bf16_ms'], row['int8_ms'], row['int8_ms'] / row['bf16_ms'], cal_ms, rel), flush=True)
        del sess, sess8
        torch.cuda.empty_cache()
    return rows


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--layers-only', action='store_true')
    ap.add_argument('--detect-only', action='store_true')
    ap.add_argument('--batches', default='16,256')
    ap.add_argument('--detect-batches', default='64,256')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    result = {}
    if not args.detect_only:
        result['layers'] = layers([int(b) for b in args.batches.split(',')])
    if not args.layers_only:
        result['detect'] = detect([int(b) for b in args.detect_batches.split(',')])
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
