"""float64 restatement of the gradient norm (train.py:432-443 calculate_gradient_norm), its tolerance, and the
inputs tests/test_gradnorm.py (CPU) and tests/test_gradnorm_gpu.py share.

Restatement: per tensor ``np.sum(g.astype(np.float64) ** 2)``, then the square root of the total.

Tolerance: ``|got - float32(ref64)| <= 1`` float32 ulp of ``ref64``, for the norm and for each squared norm.
Derived, not measured: the square of a float32 is exact in double; a double sum of n <= 2^22 terms errs by
less than n 2^-53 ~ 5e-10 relative, far below half a float32 ulp (6e-8); one final rounding follows.

Inputs: gradients are ``1e-3 randn`` with 3.0 written where a size-driven mistake would lose it -- each
tensor's last element, the first element of each second block (index 1024), and the first element of the
17th and the 33rd tensor.  A case is a list with one entry per parameter: a float32 array (its gradient;
an empty array for an empty tensor) or None (a parameter without a gradient).
"""
import math

import numpy as np

BLOCK = 1024   # kAdamPerBlock of csrc/gsr_internal.h: elements per block
TABLE = 16     # kAdamMaxTensors: tensors per launch
MARK = 3.0
SINGLE_SIZES = (1, 3, 4, 1023, 1024, 1025, 2049)
TABLE_SIZES = (5, 1023, 1, 2049, 1024, 7, 1025, 300)


def squared_norms(grads):
    """float64 squared norm of every gradient of a case (None entries skipped, as the reference skips them)."""
    return [float(np.sum(np.asarray(g).astype(np.float64) ** 2)) for g in grads if g is not None]


def gradient_norm(grads):
    """(norm, squared norms) in float64."""
    sq = squared_norms(grads)
    return math.sqrt(math.fsum(sq)), sq


def ulp32(ref64):
    """One float32 ulp of ``ref64`` (of the smallest normal number below that)."""
    return float(np.spacing(np.float32(max(abs(ref64), float(np.finfo(np.float32).tiny)))))


def ulps_off(got, ref64):
    """|got - float32(ref64)| in float32 ulps of ref64; 0 when both are the same non-finite value, inf when
    only one is non-finite or they are different ones."""
    with np.errstate(over="ignore"):  # a squared norm beyond float32 rounds to inf, as the kernel's does
        want = float(np.float32(ref64))
    got = float(got)
    if not (math.isfinite(want) and math.isfinite(got)):
        same = (math.isnan(want) and math.isnan(got)) or want == got
        return 0.0 if same else math.inf
    return abs(got - want) / ulp32(ref64)


def marked(n, rng, first=False):
    """A gradient of n elements: 1e-3 randn, MARK at the last element, at index 1024 and (``first``) at 0."""
    g = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    if n:
        g[-1] = MARK
    if n > BLOCK:
        g[BLOCK] = MARK
    if first and n:
        g[0] = MARK
    return g


def single_case(n):
    """One tensor of n elements.  The seed is one for which the inputs are fair at every size of SINGLE_SIZES
    (tests/test_gradnorm.py: the reference's float32 expression within the tolerance of float64).  That is
    a property of the seed at 2049 elements: with its two marks the reference's chain norm -> pow(2) -> sqrt,
    three float32 roundings, lands 2 or 3 ulp from float64 for about half of the seeds 0 .. 39."""
    return [marked(n, np.random.default_rng(21))]


def table_case(n):
    """``n`` non-empty tensors with gradients (sizes cycling through TABLE_SIZES), an empty tensor and a
    parameter without a gradient in the middle; the 17th and 33rd non-empty tensors carry a mark of their own."""
    rng = np.random.default_rng(100 + n)
    case = []
    for i in range(n):
        case.append(marked(TABLE_SIZES[(3 * i + i // 8) % len(TABLE_SIZES)], rng, first=i in (16, 32)))
        if i == n // 2:
            case.append(np.zeros(0, np.float32))
            case.append(None)
    return case


def two_config_case():
    """Four tensors for three param groups; groups 0 and 2 share a (betas, eps) configuration, so the
    optimizer's launches take the tensors as (0, 1, 3), (2) while the visit order is 0, 1, 2, 3."""
    rng = np.random.default_rng(7)
    return [marked(m, rng) for m in (1025, 7, 300, 2049)]


TWO_CONFIG_GROUPS = ((0, 1), (2,), (3,))
TWO_CONFIG_SETTINGS = (dict(betas=(0.9, 0.999), eps=1e-15), dict(betas=(0.8, 0.99), eps=1e-15),
                       dict(betas=(0.9, 0.999), eps=1e-15))


# ---- the mistakes the size-driven cases exist to catch, restated on the inputs ----------------------
def drop_last_partial_block(case):
    return [g if g is None else g[:g.size // BLOCK * BLOCK] for g in case]


def drop_tail_past_last_float4(case):
    return [g if g is None else g[:g.size // 4 * 4] for g in case]


def drop_after_table(case):
    """Non-empty tensors with gradients after the 16th contribute nothing."""
    out, seen = [], 0
    for g in case:
        if g is not None and g.size:
            seen += 1
            if seen > TABLE:
                g = np.zeros_like(g)
        out.append(g)
    return out


def stop_at_empty(case):
    """The walk ends at the first empty tensor."""
    k = next(i for i, g in enumerate(case) if g is not None and g.size == 0)
    return case[:k] + [None if g is None else np.zeros_like(g) for g in case[k:]]


def drop_second_configuration(case):
    first = set(TWO_CONFIG_GROUPS[0]) | set(TWO_CONFIG_GROUPS[2])
    return [g if i in first else np.zeros_like(g) for i, g in enumerate(case)]
