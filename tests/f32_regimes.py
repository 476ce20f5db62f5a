"""Value regimes for the float32 route (test_f32_regimes_host.py, test_f32_regimes_gpu.py): deterministic (Q, T) pairs of
float32 rows far off the SIFT range -- signed, offset, mixed scales, banks many binades apart, values whose squares
underflow or overflow float32, short rows, non-finite values -- and the collection case `padding_trap`.

The float32 chain is  s = fmaf(v, v, s), v = a_k - b_k, k ascending, dist = sqrtf(s)  (oracle order 1).  With rows
N(0, 1) * c the squared distance of two rows is about 256 c^2, so the chain overflows (> 3.4e38) from c ~ 1.2e18 on and
all of its terms are below float32's smallest subnormal (1.4e-45) under c ~ 1e-23."""
import numpy as np

NQ, NT, DIM = 257, 1300, 128

# Largest finite magnitude a float32 train collection, or a query bank matched against one, may hold
# (FM_COLLECTION_F32_MAX, include/fastmatch_hip.h): 2^57.
COLL_F32_MAX = np.float32(2.0 ** 57)
COLL_PAD_F32 = np.float32(1.0e18)           # what a padding row of a float32 collection holds in every dimension


def _gauss(seed, n, dim=DIM):
    return np.random.default_rng(seed).normal(0.0, 1.0, (n, dim))


def _pair(seed, scale_q=1.0, scale_t=None, dim=DIM):
    scale_t = scale_q if scale_t is None else scale_t
    Q = (_gauss(seed, NQ, dim) * scale_q).astype(np.float32)
    T = (_gauss(seed + 1, NT, dim) * scale_t).astype(np.float32)
    return Q, T


def signed():
    return _pair(100)


def offset():
    Q, T = _gauss(110, NQ), _gauss(111, NT)
    return (1000.0 + Q).astype(np.float32), (1000.0 + T).astype(np.float32)


def mixed_scale():
    """Rows that flush to zero in the fp16 planes (x 1e-6) beside rows that set the bank's scale (x 1e4)."""
    out = []
    for a in (_gauss(120, NQ), _gauss(121, NT)):
        a[::7] *= 1e4
        a[::11] *= 1e-6
        out.append(a.astype(np.float32))
    return tuple(out)


def qt_apart(binades=35):
    """Q and T `binades` powers of two apart: 35 keeps the fp16 filter usable (<= 40), 45 does not."""
    return _pair(130, 2.0 ** 20, 2.0 ** (20 - binades))


def tiny():
    return _pair(140, 1e-19)                 # squares ~1e-38: float32 subnormals


def underflow(scale=1e-23):
    return _pair(150, scale)


def huge():
    return _pair(160, 1e17)


def overflow():
    return _pair(170, 2e18)


def dim61():
    return _pair(100, dim=61)


def nonfinite():
    Q, T = signed()
    Q, T = Q.copy(), T.copy()
    T[17, 5] = np.inf
    Q[33, 100] = np.inf
    return Q, T


# name -> (builder, the fp16 filter is meant to run on a context that forces it)
REGIMES = {
    "signed": (signed, True),
    "offset": (offset, True),
    "mixed_scale": (mixed_scale, True),
    "qt_apart35": (lambda: qt_apart(35), True),
    "qt_apart45": (lambda: qt_apart(45), False),       # banks more than 40 binades apart
    "tiny": (tiny, False),                              # below the filter's value window: K5
    "underflow23": (lambda: underflow(1e-23), False),
    "underflow30": (lambda: underflow(1e-30), False),
    "huge": (huge, True),
    "overflow": (overflow, True),                       # (every distance is inf: the rescoring drops every candidate)
    "dim61": (dim61, True),
    "nonfinite": (nonfinite, False),                    # a bank with a non-finite value has no fp16 planes
}

COLLECTION_SIZES = [129, 0, 1, 127, 128, 2]             # then one image with the rest of the rows


def split_images(T, sizes=COLLECTION_SIZES, rest=True):
    images, at = [], 0
    for n in sizes:
        images.append(T[at:at + n].copy())
        at += n
    if rest:
        images.append(T[at:].copy())
    return images


def padding_trap():
    """(Q, images): images of N(0, 1) * 1e16 with 129, 1 and 127 rows; the first half of the query rows lies at
    9e17 * ones (+ noise), closer to a row of 1e18s than to any real row; the second half is like the images."""
    images = split_images((_gauss(181, 257) * 1e16).astype(np.float32), [129, 1, 127], rest=False)
    Q = _gauss(180, NQ) * 1e16
    Q[:NQ // 2] += 9e17
    return Q.astype(np.float32), images


def stack_with_padding(images, dim=DIM):
    """The rows a float32 collection holds: every non-empty image padded to whole 128-row stages with rows of 1e18.
    Returns (rows, is_padding)."""
    rows, pad = [], []
    for im in images:
        n = im.shape[0]
        if n == 0:
            continue
        n_pad = -(-n // 128) * 128
        rows.append(im)
        rows.append(np.full((n_pad - n, dim), COLL_PAD_F32, np.float32))
        pad.append(np.zeros(n, bool))
        pad.append(np.ones(n_pad - n, bool))
    return np.concatenate(rows), np.concatenate(pad)
