"""NumPy specification of the int8 inference path.  Test infrastructure only: the product never imports it.

Every step is IEEE f32 with one rounding per operation (or exact integer arithmetic), so the device is compared bit for bit.

Quantisation: symmetric int8 in -127 .. 127.
  activations  one scale per tensor, s = absmax / 127 (absmax 0 or non-finite: s = 1)
  weights      one scale per output channel over the BN-folded f32 filter W' = W * gamma / sqrt(var + eps)
  q = clip(rint(x * inv_s), -127, 127) in f32 with inv_s = float32(1) / s; NaN -> 0

Scale classes: int8 tensors connected by a pool, reorg or concat share one scale, the max of the members' abs-max; those ops are then exact on
bytes (max commutes with a monotone quantiser).  Only tensors STORED as int8 are members: the image layer runs in bf16 and its raw output is
never quantised, so the first int8 tensor -- its pooled output -- starts a class of its own.

A convolution runs in int8 when its input channel count is a multiple of 16 and it does not read the image:
  acc = exact int32 sum over taps and channels (SAME zero padding)
  t = float32(acc) * mult[n],  mult[n] = s_in * s_w[n]
  y = t + bias[n];  y = y > 0 ? y : y * alpha  (not for the linear head)
  out = int8 clip(rint(y * inv_s_out))  |  bf16 round-to-nearest-even for the head
"""
import numpy as np

F32 = np.float32
ALPHA = F32(0.1)
BN_EPS = F32(1e-5)


# ---- scalars ------------------------------------------------------------------------------------------------------------------------------

def absmax(x):
    """Largest finite |x| as f32 (0 for none) and the number of non-finite entries."""
    a = np.abs(np.asarray(x, F32)).reshape(-1)
    ok = np.isfinite(a)
    return (F32(a[ok].max()) if ok.any() else F32(0)), int((~ok).sum())


def scale_of(amax):
    a = F32(amax)
    if not np.isfinite(a) or a == 0:
        return F32(1)
    return F32(a / F32(127))


def inv_scale(s):
    return F32(F32(1) / F32(s))


def quantize(x, inv_s):
    """x: f32 array; inv_s: f32 scalar or array broadcastable against x.  -> int8"""
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.rint(np.asarray(x, F32) * np.asarray(inv_s, F32))
        q = np.clip(q, F32(-127), F32(127))
    q = np.where(np.isnan(q), F32(0), q)
    return q.astype(np.int8)


def bf16_bits(x):
    """f32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


# ---- weights ------------------------------------------------------------------------------------------------------------------------------

def fold_bn(W, gamma, beta, mean, var, eps=BN_EPS):
    """-> (W' HWIO f32, bias' f32): the operands of a batch-normalised layer with the moving statistics folded in."""
    s = (np.asarray(gamma, F32) / np.sqrt(np.asarray(var, F32) + F32(eps))).astype(F32)
    return (np.asarray(W, F32) * s).astype(F32), (np.asarray(beta, F32) - np.asarray(mean, F32) * s).astype(F32)


def quantize_weights(Wf):
    """HWIO f32 -> (int8 HWIO, per-output-channel scales f32 [cout])."""
    Wf = np.asarray(Wf, F32)
    am = np.abs(Wf).reshape(-1, Wf.shape[-1]).max(axis=0)
    s = np.array([scale_of(a) for a in am], F32)
    inv = (F32(1) / s).astype(F32)
    return quantize(Wf, inv), s


def dequantize_weights(q, s):
    return (q.astype(F32) * s).astype(F32)


# ---- ops on int8 tensors --------------------------------------------------------------------------------------------------------------------

def conv_acc(xq, wq):
    """Exact accumulators of the SAME, stride-1 convolution: xq int8 [B,H,W,C], wq int8 HWIO -> int64 [B,H,W,N].  The sums go through a
    float64 matrix product, exact below 2^53 whatever the summation order (every term is an integer of at most 2^14)."""
    kh, kw, cin, cout = wq.shape
    b, h, w, _ = xq.shape
    x = xq.astype(np.float64)
    acc = np.zeros((b, h, w, cout), np.float64)
    ph, pw = kh // 2, kw // 2
    for r in range(kh):
        for s in range(kw):
            dh, dw = r - ph, s - pw
            sh = np.zeros_like(x)
            hs, he = max(0, -dh), min(h, h - dh)
            ws, we = max(0, -dw), min(w, w - dw)
            if hs < he and ws < we:
                sh[:, hs:he, ws:we] = x[:, hs + dh:he + dh, ws + dw:we + dw]
            acc += (sh.reshape(-1, cin) @ wq[r, s].astype(np.float64)).reshape(b, h, w, cout)
    out = acc.astype(np.int64)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out


def conv_epilogue(acc, mult, bias, alpha=ALPHA, leaky=True):
    """-> y f32: two roundings, then the leaky ReLU."""
    t = (acc.astype(F32) * np.asarray(mult, F32)).astype(F32)
    y = (t + np.asarray(bias, F32)).astype(F32)
    if leaky:
        y = np.where(y > 0, y, (y * F32(alpha)).astype(F32)).astype(F32)
    return y


def max_pool(x, stride):
    """2x2 SAME max pool of an int8 (or any) NHWC array, stride 2 or 1; the window is clipped at the bottom / right edge."""
    b, h, w, c = x.shape
    oh, ow = ((h + 1) // 2, (w + 1) // 2) if stride == 2 else (h, w)
    ys = np.arange(oh) * stride
    xs = np.arange(ow) * stride
    y1, x1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
    a = x[:, ys][:, :, xs]
    bb = x[:, ys][:, :, x1]
    cc = x[:, y1][:, :, xs]
    d = x[:, y1][:, :, x1]
    return np.maximum(np.maximum(a, bb), np.maximum(cc, d))


def reorg(x):
    b, h, w, c = x.shape
    return x.reshape(b, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, h // 2, w // 2, 4 * c)


# ---- the network ----------------------------------------------------------------------------------------------------------------------------

def plan(spec, cin=3):
    """oracle.yolo2_ref op list -> nodes {kind, name, inputs, out, ...} in execution order, with readable tensor names: 'input', 'conv<i>',
    'pool<i>' (the pool behind conv<i>), 'reorg', 'concat', and 'conv' for the head."""
    nodes, cur, c, mark, last = [], 'input', cin, None, None
    for op in spec:
        if op[0] == 'conv':
            _, name, k, cout, bn = op
            nodes.append({'kind': 'conv', 'name': name, 'inputs': [cur], 'out': name, 'ksize': k, 'cin': c, 'cout': cout, 'bn': bn,
                          'int8': c % 16 == 0 and cur != 'input'})
            cur, c, last = name, cout, name
        elif op[0] == 'pool':
            out = 'pool' + last[4:]
            nodes.append({'kind': 'pool', 'name': out, 'inputs': [cur], 'out': out, 'stride': op[1]})
            cur = out
        elif op[0] == 'mark':
            mark = (cur, c)
        elif op[0] == 'reorg_concat':
            nodes.append({'kind': 'reorg', 'name': 'reorg', 'inputs': [mark[0]], 'out': 'reorg'})
            nodes.append({'kind': 'concat', 'name': 'concat', 'inputs': ['reorg', cur], 'out': 'concat'})
            cur, c = 'concat', 4 * mark[1] + c
    return nodes


def int8_tensors(nodes):
    """Names of the tensors stored as int8: whatever feeds or leaves an int8 convolution (the head's bf16 logits excepted), and what the
    byte-moving ops make of them."""
    q = set()
    for n in nodes:
        if n['kind'] == 'conv' and n['int8']:
            q.add(n['inputs'][0])
            if n['bn']:
                q.add(n['out'])
    changed = True
    while changed:
        changed = False
        for n in nodes:
            if n['kind'] in ('reorg', 'concat') or (n['kind'] == 'pool' and n['inputs'][0] in q):
                for t in n['inputs'] + [n['out']]:
                    if t not in q:
                        q.add(t)
                        changed = True
    return q


def scale_classes(nodes):
    """-> list of frozensets of int8 tensor names that share one scale."""
    q = int8_tensors(nodes)
    parent = {t: t for t in q}

    def find(t):
        while parent[t] != t:
            t = parent[t]
        return t
    for n in nodes:
        if n['kind'] in ('pool', 'reorg', 'concat'):
            members = [t for t in n['inputs'] + [n['out']] if t in q]
            for t in members[1:]:
                parent[find(t)] = find(members[0])
    classes = {}
    for t in q:
        classes.setdefault(find(t), set()).add(t)
    return sorted((frozenset(v) for v in classes.values()), key=sorted)


def resolve_scales(nodes, amax):
    """amax: {tensor name: abs-max f32} for every int8 tensor -> {tensor name: scale f32}, one value per class."""
    out = {}
    for cls in scale_classes(nodes):
        s = scale_of(max(F32(amax[t]) for t in cls))
        for t in cls:
            out[t] = s
    return out


def layer_operands(node, params, s_in):
    """-> (wq int8 HWIO, mult f32 [cout], bias f32 [cout], s_w) of an int8 convolution."""
    name = node['name']
    if node['bn']:
        Wf, bias = fold_bn(params[name + '/weights'], params[name + '/BatchNorm/gamma'], params[name + '/BatchNorm/beta'],
                           params[name + '/BatchNorm/moving_mean'], params[name + '/BatchNorm/moving_variance'])
    else:
        Wf, bias = np.asarray(params[name + '/weights'], F32), np.asarray(params[name + '/biases'], F32)
    wq, s_w = quantize_weights(Wf)
    mult = (F32(s_in) * s_w).astype(F32)
    return wq, mult, bias, s_w


def run(nodes, params, scales, start, start_q):
    """The int8 network from tensor ``start`` (int8 array ``start_q``) on.  -> {tensor name: int8 array} plus 'logits' (f32, the values the
    bf16 bit patterns in 'logits_bits' stand for)."""
    acts = {start: start_q}
    seen = False
    for n in nodes:
        if not seen:
            seen = n['out'] == start
            continue
        ins = [acts[t] for t in n['inputs']]
        if n['kind'] == 'conv':
            assert n['int8'], n['name']
            wq, mult, bias, _ = layer_operands(n, params, scales[n['inputs'][0]])
            y = conv_epilogue(conv_acc(ins[0], wq), mult, bias, leaky=n['bn'])
            if n['bn']:
                acts[n['out']] = quantize(y, inv_scale(scales[n['out']]))
            else:
                bits = bf16_bits(y)
                acts['logits_bits'] = bits
                acts['logits'] = bf16_to_f32(bits)
        elif n['kind'] == 'pool':
            acts[n['out']] = max_pool(ins[0], n['stride'])
        elif n['kind'] == 'reorg':
            acts[n['out']] = reorg(ins[0])
        elif n['kind'] == 'concat':
            acts[n['out']] = np.concatenate(ins, axis=3)
    return acts
