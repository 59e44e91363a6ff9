"""Inputs, float64 references and bounds for the distill kernel (csrc/distill.hip).  NumPy, tests/distill_ref.py and tests/head_cases.py only:
tests/test_distill_cpu.py checks the cases themselves on a machine without a GPU, tests/test_distill_gpu.py launches the kernel on them.

The reference is tests/distill_ref.py in float64 on exactly the values the kernel reads (each side rounded to bf16 first where its dtype is
bf16).  The bounds are the project's derived ones (head_cases.objective_ratio, grad_ratio) and distill_ref.accumulate_ratio.  Every case and
every reference is built once and cached; callers must not write to them."""
import functools

import numpy as np

import distill_ref as S
import head_cases as H

# name -> (B, cell_h, cell_w, A, C, ld_s, ld_t, recipe, seed): the smallest shapes at which the kernel can still go wrong
SPECS = {
    'pad3x4':    (2, 3, 4, 5, 20, 136, 125, 'randn', 41),      # a padded student row (11 padding channels), a teacher row without padding (odd ld)
    'one':       (1, 1, 1, 1, 1, 8, 6, 'randn', 42),           # one lane, one class: LPC 1, the class term is exactly 0
    'sq13':      (2, 13, 13, 5, 20, 128, 128, 'randn', 43),    # 1690 cells x 8 lanes: several workgroups and a ragged last one
    'rect9x14':  (1, 9, 14, 3, 80, 256, 256, 'randn', 44),     # cell_h != cell_w, LPC 4 with an idle lane, 80 classes
    'saturated': (2, 2, 3, 3, 4, 32, 27, 'saturated', 45),     # +-30 in every channel kind on both sides: saturated sigmoids and softmaxes
}
PAIRS = (('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32'))     # (student, teacher)
# distinct weights, so that a swapped one shows; T = 2.5 is exact in f32 and its reciprocal is not
OPTIONS = {
    'mse':          dict(weight=0.7, objectness=1.5, coords=2.0, prob=0.5),
    'kl_T2.5':      dict(weight=0.7, objectness=1.5, coords=2.0, prob=0.5, class_term='kl', temperature=2.5),
    'mse_T2.5_raw': dict(weight=1.3, objectness=0.5, coords=1.0, prob=3.0, temperature=2.5, scale_by_objectness=False),
    'kl_raw':       dict(weight=1.3, objectness=0.5, coords=1.0, prob=3.0, class_term='kl', scale_by_objectness=False),
}
KEYS = ('objectness', 'coords', 'prob')


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: B, ch, cw, A, C, D (real channels of a row), ld_s, ld_t, s and t f32 [B, cells, A, 5 + C]."""
    B, ch, cw, A, C, ld_s, ld_t, recipe, seed = SPECS[name]
    rng = np.random.RandomState(seed)
    shape = (B, ch * cw, A, 5 + C)
    if recipe == 'randn':          # a teacher and a student that agree in part, like two networks trained on the same data
        t = rng.randn(*shape) * 1.2
        s = 0.5 * t + rng.randn(*shape) * 0.9
    elif recipe == 'saturated':    # every value +30, -30 or an ordinary one, independently on both sides, so that every channel kind sees every pairing
        pick = lambda: np.where(rng.rand(*shape) < 0.7, rng.choice([-30.0, 30.0], shape), rng.randn(*shape))
        s, t = pick(), pick()
        for k in range(5 + C):     # ... and the first lanes hold the four saturated pairings in every channel for certain
            s.reshape(-1, 5 + C)[:4, k] = [30, 30, -30, -30]
            t.reshape(-1, 5 + C)[:4, k] = [30, -30, 30, -30]
    else:
        raise KeyError(recipe)
    s, t = s.astype(np.float32), t.astype(np.float32)
    s.setflags(write=False), t.setflags(write=False)
    return dict(name=name, B=B, ch=ch, cw=cw, A=A, C=C, D=A * (5 + C), ld_s=ld_s, ld_t=ld_t, s=s, t=t)


def read64(name, pair):
    """(s, t) as the kernel reads them, widened to float64."""
    c = case(name)
    return H.inputs64(c['s'], pair[0]), H.inputs64(c['t'], pair[1])


@functools.lru_cache(maxsize=None)
def reference(name, pair, options, mutation=None):
    """(objectives dict, g float64 [B, cells, A, 5 + C]) of the specification for case `name`, dtypes `pair`, OPTIONS[options]."""
    s, t = read64(name, pair)
    obj, g = S.loss(s, t, mutation=mutation, **OPTIONS[options])
    g.setflags(write=False)
    return obj, g


@functools.lru_cache(maxsize=None)
def start_gradient(name, mode):
    """The d0 of the accumulation checks: what a loss launch could have left in dlogits, random, already in the student's dtype (f32 values)."""
    c = case(name)
    d0 = (np.random.RandomState(1000 + SPECS[name][8]).randn(*c['s'].shape) * 1e-2).astype(np.float32)
    d0 = H.inputs64(d0, mode).astype(np.float32)
    d0.setflags(write=False)
    return d0


def worst_ratio(name, pair, options, obj, g):
    """max over the objectives' and the zero-start gradient's |err| / bound of a candidate (obj dict, exact gradient g) against the specification: what a
    kernel that computed `g` exactly and stored it in the student's dtype would score."""
    ref_obj, ref_g = reference(name, pair, options)
    ratios = [H.objective_ratio(obj[k], ref_obj[k]) for k in KEYS if ref_obj[k] != 0 or obj[k] != 0]
    ratios.append(H.grad_ratio(H.stored(g, pair[0]), ref_g, pair[0]))
    return max(ratios)
