"""Matching for descriptors that are already on the GPU: CUDA tensors in, CUDA tensors out.

``matchutil`` mirrors the reference, whose descriptors are NumPy arrays from OpenCV on the CPU.  A pipeline whose extractor
runs on the GPU (a PyTorch-ROCm model) holds its descriptors as device tensors; the functions here hand their memory to the
library as it is (``fm_bank_create_dev``: the preparation kernels read the tensor in place, rows ``stride(0)`` apart) and
leave the results in tensors the library's kernels write directly (``fm_knn_dev`` / ``fm_xcheck1_dev`` /
``fm_knn2_ratio_dev``).  Nothing crosses PCIe.

* ``bank(tensor, *, binary=False, hamming2=False, float_route=False, context=None)`` -- a resident ``Bank`` from a 2-D CUDA tensor of dtype
  uint8, float32, float16 or bfloat16 (``binary``: uint8 rows of 1 .. 64 packed bytes for Hamming distance).  On return the
  tensor may be overwritten.  ``hamming2``: the same rows for NORM_HAMMING2 (ORB with WTA_K = 3 or 4: the distance counts the
  2-bit cells that differ); ``knn``, ``mutual_nn``, ``ratio_match``, ``mutual_ratio_match`` and ``hamming_radius_match`` take
  two such resident banks, ``Collection.add``, a collection query and every masked call refuse them with ``ValueError``.
* ``knn(q, t, k, mask=None)`` -> ``(idx int32 [nq, k], dist float32 [nq, k])``, 1 <= k <= 8.  ``mask``: a CUDA ``bool`` /
  ``uint8`` tensor ``[nq, nt]``, nonzero = the pair may be matched (cv2's ``knnMatch(q, t, k, mask)``), or a resident
  ``_ffi.Mask``; rows may be pitched (a column slice of a wider tensor).  It is packed into the library's bit mask on the
  device, read in place behind the current stream (``fm_mask_set_dev``): no host copy.
* ``mutual_nn(q, t)`` -> ``(tidx int32 [nq], dist float32 [nq])``: the cross-checked 1-NN (-1 / inf: unmatched).
* ``ratio_match(q, t, tau)`` -> ``(qidx, tidx, dist)`` of the rows whose first / second distance is below ``tau``.
* ``mutual_ratio_match(q, t, tau, symmetric=False)`` -> ``(qidx, tidx, dist)`` of the rows that pass the ratio test AND are the
  nearest query row of their first neighbour (hloc's "NN-ratio + mutual", kornia's ``match_smnn``); ``symmetric``: the train
  row's own 2-NN list over the query rows passes the ratio test too (``fm_mutual_ratio_dev``).
* ``radius_match(q, t, r)`` -> ``(offsets int64 [nq + 1], idx int32 [n], dist float32 [n])``: every train row with distance
  < r per query row (``cv2.BFMatcher.radiusMatch``), row i's list at ``offsets[i]:offsets[i + 1]``, ascending (distance, index).
  ``r`` is a Python or NumPy scalar, or a float32 CUDA tensor ``[nq]`` of one radius per query row on the context's device
  (``tau * selfdist`` as it comes out of a kernel), read in place (``fm_radius_match_dev``).
* ``hamming_radius_match(q, t, r)`` -> the same three tensors for BINARY descriptors (uint8 CUDA tensors of 1 .. 64 packed
  bytes per row, or binary ``Bank``s): every train row with ``popcount(q XOR t) < r`` (strict, float32 -- ``h <= H`` is
  ``r = H + 0.5``), ascending (h, index); ``r`` as in ``radius_match`` (``fm_hamming_radius_match_dev``).  ``radius_match``
  itself stays the L2 call.
* ``hamming_fast_match(q, t, tau)`` -> ``(rows int32 [m, 3], count int64 [1])``: Fast-Match's accepted-match test on binary
  descriptors -- (query, train row, float32 bits of ``popcount(q XOR t)``) of the cross-checked nearest neighbours with
  ``dist / selfdist(q) < tau``; the query's Hamming self distances are computed on the device when its bank carries none
  (``fm_hamming_self_dist_batch``, ``fm_hamming_match_accepted_dev``).

* ``Collection(context=None)`` -- a train collection (``cv2.BFMatcher.add`` / ``train``) whose images are CUDA tensors: the
  retrieval flow extract -> ``add`` to the database -> query -> consume without a copy to the host.  A context manager.
  ``add(tensor, *, binary=False)`` reads the tensor in place (``fm_collection_add_dev``) and returns the image index;
  ``knn(q, k, masks=None)`` -> ``(img, idx, dist)`` [nq, k] (``masks``: one CUDA ``bool`` / ``uint8`` tensor ``[nq, rows of the
  image]`` per added image, ``None`` entries permit everything -- cv2's ``knnMatch(q, k, masks=[...])``; or a resident
  ``_ffi.Mask`` from ``Collection.mask``); ``ratio_match(q, tau)`` -> ``(qidx, img, tidx, dist)``;
  ``radius_match(q, r)`` -> ``(offsets, img, idx, dist)``, ``r`` as in the module's ``radius_match``;
  ``hamming_radius_match(q, r)`` -> the same against a binary collection (``fm_collection_hamming_radius_match_dev``);
  ``fast_match_each(q, tau, cap=None)`` -> ``(rows int32 [n_images, cap, 3], counts int64 [n_images])``, the accepted-match
  test inside every image (``q``: a ``Bank`` carrying self distances, ``Context.self_dist_batch([q], want_host=False)``);
  ``hamming_fast_match_each(q, tau, cap=None)`` -> the same two tensors on a binary collection (``q``: a binary ``Bank``
  carrying Hamming self distances, ``Context.hamming_self_dist_batch``);
  ``mutual_nn_each(q, max_dist=None, cap=None)`` -> the same two tensors for the cross-checked 1-NN inside every image
  (``cv2.BFMatcher(norm, crossCheck=True).match(q, image)`` image by image, kept while ``dist < max_dist``), on uint8,
  float and binary collections alike;
  ``mutual_ratio_each(q, tau, symmetric=False, cap=None)`` -> the same two tensors for ``mutual_ratio_match`` inside every
  image (``fm_collection_mutual_ratio_each_dev``: one restricted reverse sweep serves all images);
  ``match_pairs(pairs=None, tau=0.8, symmetric=False, cap=None)`` -> ``(offsets int64 [n_pairs + 1], rows int32 [n, 3])``: the
  images matched against EACH OTHER, ``mutual_ratio_match(image_a, image_b)`` for every ordered pair (a, b) of ``pairs`` (a
  host sequence or an int32 CPU tensor; None: every a < b) in one call (``fm_collection_pairs_mutual_ratio_dev``), no host
  wait unless ``cap`` is None (then one, for the total that sizes ``rows``);
  ``clear()``, ``close()``, ``info()``.  The collection equals the ``_ffi.Collection`` the same values build on the host.

Wide float descriptors -- ``[n, 129 .. 256]`` float32 / float16 / bfloat16 tensors, SuperPoint's 256-D rows for one -- make
wide float banks (``FM_BANK_F32W``): ``bank``, ``knn`` with k <= 2, ``mutual_nn``, ``ratio_match`` and ``mutual_ratio_match``
take them; ``radius_match``, a masked or k >= 3 ``knn`` and ``Collection.add`` raise ``ValueError`` before the library is
touched.  Their match graph: ``Collection.add_wide(tensor)`` (``fm_collection_add_wide_dev``) makes a WIDE collection, which
takes no other images and serves ``match_pairs``, ``info``, ``clear`` and ``close``; its other methods raise ``ValueError``.
A wide QUERY against a wide collection, image by image: ``Collection.wide_mutual_ratio_each(q, tau, symmetric=False,
cap=None)`` -> ``(offsets int64 [n_images + 1], rows int32 [n, 3] = (query row, row inside the image, float32 distance
bits))``, image i equal to ``mutual_ratio_match(q, image_i)`` (``fm_collection_wide_mutual_ratio_each_dev``; the
visual-localisation pattern); ``cap`` as in ``match_pairs``.
Fast-Match's self-distance test on wide descriptors: ``wide_fast_match(q, t, tau)`` -> ``(rows int32 [m, 3], count int64
[1])`` (``fm_wide_self_dist_batch``, ``fm_wide_match_accepted_dev``) and, against a wide collection image by image,
``Collection.wide_fast_match_each(q, tau, cap=None)`` -> ``(rows int32 [n_images, cap, 3], counts int64 [n_images])``
(``fm_collection_wide_match_accepted_each_dev``).
knnMatch under a mask on wide descriptors: ``wide_knn_masked(q, t, k, mask)`` -> ``(idx int32 [nq, k], dist float32 [nq, k])``,
k = 1 or 2, ``mask`` as in ``knn`` (``fm_wide_knn_masked_dev``, on the matrix cores); ``knn`` keeps refusing the combination.

``q`` and ``t`` are ``Bank``s or CUDA tensors (a tensor becomes a bank for the call).  The values are those of
``Context.knn`` / ``xcheck1`` / ``knn2_ratio`` on banks built from the same numbers on the host, bit for bit.

Streams: ``torch.cuda.current_stream()`` is both the producer of the descriptor tensors and the consumer of the results --
the library orders its kernels behind the one and the stream behind the other on the device, so no ``synchronize()`` is needed
on either side (``ratio_match`` and ``Collection.ratio_match`` read the accepted count back to size their outputs: one host
wait; ``mutual_ratio_match`` and ``Collection.mutual_ratio_each`` wait once inside the library, for the number of rows that
passed the ratio test, which sizes the restricted reverse sweep, and ``mutual_ratio_match`` once more for its count; ``radius_match`` and ``Collection.radius_match`` likewise wait for the total that sizes theirs -- a counts call, then a
fill call -- and the library reads the per-row counts back to plan its chunks).  For the radius calls the current stream is
also the producer of ``r``.

``torch`` is imported inside the functions: importing the package does not need it.  A CPU tensor, another dtype or
another rank raises ``ValueError`` before the library is touched -- for a radius tensor: a CPU tensor, a dtype other than
float32, a shape other than ``[nq]``, another device.  Tensors must live on the context's device.
"""
import numpy as np

from . import _ffi

_DTYPES = {"torch.uint8": _ffi.FM_DT_U8, "torch.float32": _ffi.FM_DT_F32, "torch.float16": _ffi.FM_DT_F16,
           "torch.bfloat16": _ffi.FM_DT_BF16}


def _checked(tensor, binary=False, hamming2=False):
    """(tensor with unit column stride, FM_DT_*) or ValueError -- before anything reaches the library."""
    import torch
    if not isinstance(tensor, torch.Tensor):
        raise ValueError("descriptors must be a torch.Tensor or a resident Bank, got %s" % type(tensor).__name__)
    if not tensor.is_cuda:
        raise ValueError("descriptors must be a CUDA tensor (a host array goes to Context.bank / matchutil)")
    if tensor.dim() != 2:
        raise ValueError("descriptors must be 2-D [n, dim], got %d-D" % tensor.dim())
    dt = _DTYPES.get(str(tensor.dtype))
    if dt is None:
        raise ValueError("descriptor dtype %s: uint8, float32, float16 or bfloat16 are taken" % tensor.dtype)
    if binary and hamming2:
        raise ValueError("binary (NORM_HAMMING) and hamming2 (NORM_HAMMING2) are two norms: ask for one")
    if binary or hamming2:
        if dt != _ffi.FM_DT_U8:
            raise ValueError("binary descriptors must be uint8 (packed bits), got %s" % tensor.dtype)
        if hamming2 and not 1 <= tensor.shape[1] <= 64:
            raise ValueError("NORM_HAMMING2 descriptors have 1 .. 64 bytes per row, got %d" % tensor.shape[1])
        dt = _ffi.FM_DT_BIN2 if hamming2 else _ffi.FM_DT_BIN
    if tensor.shape[1] < 1:
        raise ValueError("descriptors must have at least one column")
    # rows may be pitched (a column slice of a wider tensor); elements of a row must be adjacent.  (A one-row or empty
    # tensor can report any row stride: below the row size it is made dense.)
    if tensor.stride(1) != 1 or tensor.stride(0) < tensor.shape[1]:
        tensor = tensor.contiguous()
    return tensor, dt


def _refuse_wide(who, what, *operands):
    """ValueError before the library is touched: wide float descriptors (129 .. 256 values per row -- a resident FM_BANK_F32W
    bank or a float tensor of that width) are served by ``bank``, ``knn`` with k <= 2, ``mutual_nn``, ``ratio_match`` and
    ``mutual_ratio_match`` only."""
    for x in operands:
        if isinstance(x, _ffi.Bank):
            wide = x.kind == _ffi.FM_BANK_F32W
        else:
            shape = getattr(x, "shape", ())
            wide = len(shape) == 2 and shape[1] > 128 and str(getattr(x, "dtype", "")) != "torch.uint8"
        if wide:
            raise ValueError("%s: %s is not built for wide float descriptors (129 .. 256 values per row: knn with k <= 2, "
                             "mutual_nn, ratio_match and mutual_ratio_match are)" % (who, what))


def _refuse_hamming2(who, what, *operands):
    """ValueError before the library is touched: a NORM_HAMMING2 bank (``bank(tensor, hamming2=True)``) is served by ``knn``,
    ``mutual_nn``, ``ratio_match``, ``mutual_ratio_match`` and ``hamming_radius_match`` without a mask, and by nothing else."""
    if any(isinstance(x, _ffi.Bank) and x.kind == _ffi.FM_BANK_BIN2 for x in operands):
        raise ValueError("%s: %s is not built for NORM_HAMMING2 banks (knn, mutual_nn, ratio_match, mutual_ratio_match and "
                         "hamming_radius_match without a mask are)" % (who, what))


def _checked_mask(m, nq, nt, what="mask"):
    """A mask tensor with unit column stride, viewed as uint8 -- or ValueError, before anything reaches the library."""
    import torch
    if not isinstance(m, torch.Tensor):
        raise ValueError("%s must be a CUDA bool / uint8 tensor or a resident Mask, got %s" % (what, type(m).__name__))
    if not m.is_cuda:
        raise ValueError("%s must be a CUDA tensor (a host array goes to Mask.set / matchutil's options['mask'])" % what)
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s dtype %s: bool or uint8 are taken" % (what, m.dtype))
    if m.dim() != 2 or tuple(m.shape) != (nq, nt):
        raise ValueError("%s must be [%d, %d] (query rows, train rows), got %s" % (what, nq, nt, tuple(m.shape)))
    if nq and nt and (m.stride(1) != 1 or m.stride(0) < nt):
        m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _set_mask(mask, m, img):
    """One image's bits from a checked tensor, read in place behind the current stream of its device."""
    import torch
    if m.shape[0] == 0 or m.shape[1] == 0:
        return
    with torch.cuda.device(m.device):
        stream = torch.cuda.current_stream().cuda_stream
    mask.set_dev(m.data_ptr(), img=img, pitch=m.stride(0), stream=stream)


def _rows_hint(x):
    return x.n if isinstance(x, _ffi.Bank) else (x.shape[0] if hasattr(x, "shape") and len(x.shape) == 2 else -1)


def _pair_mask_checked(mask, q, t):
    """``mask`` of a pair call before anything is uploaded: None, a resident Mask as it is, or a checked tensor."""
    if mask is None or isinstance(mask, _ffi.Mask):
        return mask
    return _checked_mask(mask, _rows_hint(q), _rows_hint(t))


def _pair_mask(mask, qb, tb, made):
    """The resident Mask of a checked pair mask (a tensor's is made for this call and closed with ``made``)."""
    if isinstance(mask, _ffi.Mask):
        return mask
    mk = qb.ctx.mask(qb.n, tb.n)
    made.append(mk)
    _set_mask(mk, mask, 0)
    return mk


def _ctx_for(tensor, context):
    return context if context is not None else _ffi.default_context(tensor.device.index)


def bank(tensor, *, binary=False, hamming2=False, float_route=False, context=None):
    """A resident ``Bank`` from a CUDA tensor, read in place behind the current stream's work (module docstring).
    ``hamming2``: uint8 rows of 1 .. 64 packed bytes whose elements are 2-bit values, for NORM_HAMMING2 (``FM_DT_BIN2``)."""
    import torch
    tensor, dt = _checked(tensor, binary, hamming2)
    ctx = _ctx_for(tensor, context)
    n, dim = tensor.shape
    with torch.cuda.device(tensor.device):
        stream = torch.cuda.current_stream().cuda_stream
    return ctx.bank_from_device(tensor.data_ptr() if n else 0, dt, n, dim, tensor.stride(0) * tensor.element_size(),
                                float_route=float_route, stream=stream)


def _pair(q, t):
    """Both operands as banks of one context; [banks made for this call]."""
    ctx = next((x.ctx for x in (q, t) if isinstance(x, _ffi.Bank)), None)
    checked = [x if isinstance(x, _ffi.Bank) else _checked(x) for x in (q, t)]      # (every refusal before any upload)
    made = []
    out = []
    for x in checked:
        if isinstance(x, _ffi.Bank):
            out.append(x)
            continue
        b = bank(x[0], context=ctx)
        ctx = b.ctx
        made.append(b)
        out.append(b)
    return out[0], out[1], made


def _stream_and_device(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        return torch.cuda.current_stream().cuda_stream, dev


def knn(q, t, k, mask=None):
    """k nearest train rows of every query row: ``(idx int32 [nq, k], dist float32 [nq, k])`` CUDA tensors, ascending
    (distance, train index); -1 / inf where ``t`` has fewer than k rows.  1 <= k <= 8.  ``mask`` (module docstring): only the
    pairs it permits are candidates (``fm_knn_masked_dev``)."""
    import torch
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    if mask is not None:
        _refuse_wide("knn", "a mask", q, t)
        _refuse_hamming2("knn", "a mask", q, t)
    if k > 2:
        _refuse_wide("knn", "k >= 3", q, t)
    if mask is not None and not isinstance(mask, _ffi.Mask):
        nq, nt = (x.n if isinstance(x, _ffi.Bank) else (x.shape[0] if hasattr(x, "shape") and len(x.shape) == 2 else -1) for x in (q, t))
        mask = _checked_mask(mask, nq, nt)
    qb, tb, made = _pair(q, t)
    try:
        stream, dev = _stream_and_device(qb.ctx)
        idx = torch.empty((qb.n, k), dtype=torch.int32, device=dev)
        dist = torch.empty((qb.n, k), dtype=torch.float32, device=dev)
        if mask is None:
            qb.ctx.knn_dev(qb, tb, k, idx.data_ptr() if qb.n else 0, dist.data_ptr() if qb.n else 0, consumer_stream=stream)
            return idx, dist
        mk = mask
        if not isinstance(mask, _ffi.Mask):
            mk = qb.ctx.mask(qb.n, tb.n)
            made.append(mk)
            _set_mask(mk, mask, 0)
        qb.ctx.knn_masked_dev(qb, tb, mk, k, idx.data_ptr() if qb.n else 0, dist.data_ptr() if qb.n else 0, consumer_stream=stream)
        return idx, dist
    finally:
        for b in made:
            b.close()


def mutual_nn(q, t):
    """Cross-checked 1-NN (``cv2.BFMatcher(..., crossCheck=True)``): ``(tidx int32 [nq], dist float32 [nq])``."""
    import torch
    qb, tb, made = _pair(q, t)
    try:
        stream, dev = _stream_and_device(qb.ctx)
        tidx = torch.empty(qb.n, dtype=torch.int32, device=dev)
        dist = torch.empty(qb.n, dtype=torch.float32, device=dev)
        qb.ctx.xcheck1_dev(qb, tb, tidx.data_ptr() if qb.n else 0, dist.data_ptr() if qb.n else 0, consumer_stream=stream)
        return tidx, dist
    finally:
        for b in made:
            b.close()


def ratio_match(q, t, tau):
    """The classic ratio match: ``(qidx int32 [m], tidx int32 [m], dist float32 [m])`` of the query rows whose nearest /
    second nearest distance is below ``tau`` (float64; a zero second distance is rejected), ascending query index."""
    import torch
    qb, tb, made = _pair(q, t)
    try:
        stream, dev = _stream_and_device(qb.ctx)
        cap = qb.n
        rows = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        m = qb.ctx.knn2_ratio_dev(qb, tb, float(tau), rows.data_ptr(), count.data_ptr(), cap, want_count=True,
                                  consumer_stream=stream)
        rows = rows[:min(m, cap)]
        return rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous().view(torch.float32)
    finally:
        for b in made:
            b.close()


def mutual_ratio_match(q, t, tau, symmetric=False):
    """Mutual nearest neighbours that pass the ratio test: ``(qidx int32 [m], tidx int32 [m], dist float32 [m])`` of the query
    rows i with d0 / d1 < ``tau`` (float64; a zero second distance is rejected) whose first neighbour's nearest query row is i
    (lowest index on ties); ``symmetric``: that train row's 2-NN list over the query rows passes the same test.  Ascending
    query index.  Two host waits: the candidate count inside the library, the accepted count that sizes the outputs."""
    import torch
    qb, tb, made = _pair(q, t)
    try:
        stream, dev = _stream_and_device(qb.ctx)
        cap = qb.n
        rows = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        m = qb.ctx.mutual_ratio_dev(qb, tb, float(tau), bool(symmetric), rows.data_ptr(), count.data_ptr(), cap, want_count=True,
                                    consumer_stream=stream)
        rows = rows[:min(m, cap)]
        return rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous().view(torch.float32)
    finally:
        for b in made:
            b.close()


def _rows_and_device(q):
    """(query rows, device index) of a bank or a descriptor tensor -- nothing reaches the library."""
    if isinstance(q, _ffi.Bank):
        return q.n, q.ctx.device
    t, _ = _checked(q)
    return t.shape[0], t.device.index


def _radius(r, nq, device):
    """(float32 CUDA tensor [nq] or None, scalar radius) or ValueError -- before anything reaches the library."""
    import torch
    if not isinstance(r, torch.Tensor):
        if np.ndim(r) != 0:
            raise ValueError("a radius per query row must be a float32 CUDA tensor [nq] (a host array goes to Context.radius_match)")
        return None, float(np.float32(r))
    if r.dtype != torch.float32:
        raise ValueError("radius dtype %s: a radius tensor must be float32" % r.dtype)
    if r.dim() != 1:
        raise ValueError("a radius tensor must be 1-D [nq], got %d-D" % r.dim())
    if r.shape[0] != nq:
        raise ValueError("%d radii for %d query rows" % (r.shape[0], nq))
    if not r.is_cuda:
        raise ValueError("a radius tensor must be a CUDA tensor (a host array goes to Context.radius_match)")
    if device is not None and r.device.index != device:
        raise ValueError("the radius tensor lives on device %s, the context on device %s" % (r.device.index, device))
    return r.contiguous(), 0.0


def _radius_lists(call, nq, rad, r_all, stream, dev, with_img):
    """The counts call, then the fill call, of a ``radius_match_dev`` (``call(radius_ptr, radius_all, cap, offsets_ptr, list
    pointers ...)``): device tensors (offsets, [img,] idx, dist)."""
    import torch
    nl = 3 if with_img else 2
    offsets = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    rp = rad.data_ptr() if rad is not None and nq else 0
    total = call(rp, r_all, 0, offsets.data_ptr(), *([0] * nl), consumer_stream=stream)
    lists = [torch.empty(total, dtype=torch.int32, device=dev) for _ in range(nl - 1)]
    lists.append(torch.empty(total, dtype=torch.float32, device=dev))
    if total > 0:
        again = call(rp, r_all, total, offsets.data_ptr(), *[x.data_ptr() for x in lists], consumer_stream=stream)
        if again != total:
            raise _ffi.FastMatchHipError("radius_match: %d entries on the second call, %d on the first" % (again, total))
    return (offsets,) + tuple(lists)


def radius_match(q, t, r, mask=None):
    """``cv2.BFMatcher.radiusMatch``: ``(offsets int64 [nq + 1], idx int32 [n], dist float32 [n])`` CUDA tensors, every train
    row with distance < r per query row, ascending (distance, train index).  ``r``: a scalar, or a float32 CUDA tensor [nq]
    read in place behind the current stream's work (module docstring).  One host wait for the total.  ``mask`` (a bool / uint8
    CUDA tensor [nq, nt] or a resident Mask, as in ``knn``): the same lists without the pairs it forbids
    (``fm_radius_match_masked_dev``)."""
    _refuse_wide("radius_match", "radiusMatch", q, t)
    _refuse_hamming2("radius_match", "the L2 radiusMatch (hamming_radius_match is the call)", q, t)
    nq, device = _rows_and_device(q)
    if not isinstance(t, _ffi.Bank):
        _checked(t)
    rad, r_all = _radius(r, nq, device)
    mask = _pair_mask_checked(mask, q, t)
    qb, tb, made = _pair(q, t)
    try:
        stream, dev = _stream_and_device(qb.ctx)
        if mask is not None:
            mk = _pair_mask(mask, qb, tb, made)
            return _radius_lists(lambda *a, **k: qb.ctx.radius_match_masked_dev(qb, tb, mk, *a, **k), qb.n, rad, r_all, stream, dev, False)
        return _radius_lists(lambda *a, **k: qb.ctx.radius_match_dev(qb, tb, *a, **k), qb.n, rad, r_all, stream, dev, False)
    finally:
        for b in made:
            b.close()


def _binary_operand(who, x, hamming2_ok=False):
    """A binary bank as it is, or a checked uint8 tensor of 1 .. 64 bytes per row -- ValueError before the library is touched."""
    if isinstance(x, _ffi.Bank):
        if x.kind != _ffi.FM_BANK_BIN and not (hamming2_ok and x.kind == _ffi.FM_BANK_BIN2):
            raise ValueError("%s takes binary banks (bank(tensor, binary=True)); radius_match is the L2 call" % who)
        return x
    t, _ = _checked(x, binary=True)
    if t.shape[1] > 64:
        raise ValueError("%s: binary descriptors have 1 .. 64 bytes per row, got %d" % (who, t.shape[1]))
    return t


def hamming_radius_match(q, t, r, mask=None):
    """``mask`` as in ``radius_match``.
    ``cv2.BFMatcher(NORM_HAMMING).radiusMatch`` on binary descriptors: ``(offsets int64 [nq + 1], idx int32 [n], dist
    float32 [n])`` CUDA tensors, every train row with ``popcount(q XOR t) < r`` per query row (strict, float32: ``h <= H`` is
    ``r = H + 0.5``), ascending (h, train index).  ``q`` / ``t``: uint8 CUDA tensors of packed bits or binary ``Bank``s;
    ``r`` as in ``radius_match``.  One host wait for the total.  Two NORM_HAMMING2 banks (``bank(tensor, hamming2=True)``): the
    same lists under the cell count of NORM_HAMMING2, without a mask."""
    who = "hamming_radius_match"
    ops = [_binary_operand(who, x, hamming2_ok=True) for x in (q, t)]
    if any(isinstance(x, _ffi.Bank) and x.kind == _ffi.FM_BANK_BIN2 for x in ops):
        # NORM_HAMMING2: two resident banks of that kind (a tensor is a NORM_HAMMING operand), the radius against the cell count
        if not all(isinstance(x, _ffi.Bank) and x.kind == _ffi.FM_BANK_BIN2 for x in ops):
            raise ValueError("%s: a NORM_HAMMING2 bank pairs with another NORM_HAMMING2 bank only (bank(tensor, hamming2=True))" % who)
        if mask is not None:
            _refuse_hamming2(who, "a mask", *ops)
    widths = [x.dim if isinstance(x, _ffi.Bank) else x.shape[1] for x in ops]
    if widths[0] != widths[1]:
        raise ValueError("%s: %d bytes per query row, %d per train row" % (who, widths[0], widths[1]))
    nq = ops[0].n if isinstance(ops[0], _ffi.Bank) else ops[0].shape[0]
    ctx = next((x.ctx for x in ops if isinstance(x, _ffi.Bank)), None)
    rad, r_all = _radius(r, nq, ctx.device if ctx is not None else ops[0].device.index)
    mask = _pair_mask_checked(mask, ops[0], ops[1])
    made, banks = [], []
    try:
        for x in ops:
            if not isinstance(x, _ffi.Bank):
                x = bank(x, binary=True, context=ctx)
                ctx = x.ctx
                made.append(x)
            banks.append(x)
        qb, tb = banks
        stream, dev = _stream_and_device(qb.ctx)
        if mask is not None:
            mk = _pair_mask(mask, qb, tb, made)
            return _radius_lists(lambda *a, **k: qb.ctx.radius_match_masked_dev(qb, tb, mk, *a, **k), qb.n, rad, r_all, stream, dev, False)
        return _radius_lists(lambda *a, **k: qb.ctx.hamming_radius_match_dev(qb, tb, *a, **k), qb.n, rad, r_all, stream, dev, False)
    finally:
        for b in made:
            b.close()


def hamming_fast_match(q, t, tau):
    """Fast-Match's accepted-match test on binary descriptors, left on the device: ``(rows int32 [m, 3] = (query, train row,
    float32 bits of popcount(q XOR t)), count int64 [1])`` CUDA tensors, ascending query index -- t is the cross-checked
    nearest neighbour of q and ``dist / selfdist(q) < tau``, selfdist(q) the Hamming distance from q to its nearest OTHER
    query row (a row with a duplicate is never accepted).  ``q`` / ``t``: uint8 CUDA tensors of packed bits or binary
    ``Bank``s; a query bank that carries no self distances gets them on the device (``fm_hamming_self_dist_batch``).  One host
    wait, for the count that sizes ``rows``."""
    import torch
    who = "hamming_fast_match"
    ops = [_binary_operand(who, x) for x in (q, t)]
    widths = [x.dim if isinstance(x, _ffi.Bank) else x.shape[1] for x in ops]
    if widths[0] != widths[1]:
        raise ValueError("%s: %d bytes per query row, %d per train row" % (who, widths[0], widths[1]))
    ctx = next((x.ctx for x in ops if isinstance(x, _ffi.Bank)), None)
    made, banks = [], []
    try:
        for x in ops:
            if not isinstance(x, _ffi.Bank):
                x = bank(x, binary=True, context=ctx)
                ctx = x.ctx
                made.append(x)
            banks.append(x)
        qb, tb = banks
        if not qb.has_selfdist:
            qb.ctx.hamming_self_dist_batch([qb], want_host=False)
        _, dev = _stream_and_device(qb.ctx)
        cap = qb.n
        rows = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        # (the call runs on the context's stream and returns when it is done: the fresh tensors must be ours by then)
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()
        m = qb.ctx.hamming_match_accepted_dev(qb, tb, float(tau), rows.data_ptr(), count.data_ptr(), cap)
        return rows[:min(m, cap)], count
    finally:
        for b in made:
            b.close()


def _wide_operand(who, x):
    """A wide float bank as it is, or a checked float32 / float16 / bfloat16 tensor of 129 .. 256 values per row -- ValueError
    before the library is touched."""
    if isinstance(x, _ffi.Bank):
        if x.kind != _ffi.FM_BANK_F32W:
            raise ValueError("%s takes wide float banks (FM_BANK_F32W, 129 .. 256 values per row); fast matching of the other "
                             "kinds goes through Context.match_accepted_dev / hamming_fast_match" % who)
        return x
    t, dt = _checked(x)
    if dt == _ffi.FM_DT_U8 or not 129 <= t.shape[1] <= 256:
        raise ValueError("%s: wide descriptors are float32 / float16 / bfloat16 tensors of 129 .. 256 values per row, got %s "
                         "[%d, %d]" % (who, t.dtype, t.shape[0], t.shape[1]))
    return t


def wide_fast_match(q, t, tau):
    """Fast-Match's accepted-match test on wide float descriptors (129 .. 256 values per row), left on the device: ``(rows
    int32 [m, 3] = (query, train row, float32 distance bits), count int64 [1])`` CUDA tensors, ascending query index -- t is
    the cross-checked nearest neighbour of q and ``dist / selfdist(q) < tau``, selfdist(q) the distance from q to its nearest
    OTHER query row (a row with an exact duplicate is never accepted).  ``q`` / ``t``: float32 / float16 / bfloat16 CUDA
    tensors (half and bfloat16 widened exactly) or wide ``Bank``s; a query bank that carries no self distances gets them on
    the device (``fm_wide_self_dist_batch``).  One host wait, for the count that sizes ``rows``."""
    import torch
    who = "wide_fast_match"
    ops = [_wide_operand(who, x) for x in (q, t)]
    widths = [x.dim if isinstance(x, _ffi.Bank) else x.shape[1] for x in ops]
    if widths[0] != widths[1]:
        raise ValueError("%s: %d values per query row, %d per train row" % (who, widths[0], widths[1]))
    ctx = next((x.ctx for x in ops if isinstance(x, _ffi.Bank)), None)
    made, banks = [], []
    try:
        for x in ops:
            if not isinstance(x, _ffi.Bank):
                x = bank(x, context=ctx)
                ctx = x.ctx
                made.append(x)
            banks.append(x)
        qb, tb = banks
        if not qb.has_selfdist:
            qb.ctx.wide_self_dist_batch([qb], want_host=False)
        _, dev = _stream_and_device(qb.ctx)
        cap = qb.n
        rows = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        # (the call runs on the context's stream and returns when it is done: the fresh tensors must be ours by then)
        with torch.cuda.device(dev):
            torch.cuda.current_stream().synchronize()
        m = qb.ctx.wide_match_accepted_dev(qb, tb, float(tau), rows.data_ptr(), count.data_ptr(), cap)
        return rows[:min(m, cap)], count
    finally:
        for b in made:
            b.close()


def wide_knn_masked(q, t, k, mask):
    """``knn(q, t, k, mask)`` on wide float descriptors (129 .. 256 values per row), k = 1 or 2, on the matrix cores: ``(idx int32
    [nq, k], dist float32 [nq, k])`` CUDA tensors, ``knn``'s lists for the pair computed over the train rows ``mask`` permits per
    query row -- the same distance bits; -1 / inf where fewer than k rows are permitted (``fm_wide_knn_masked_dev``).  ``q`` /
    ``t``: float32 / float16 / bfloat16 CUDA tensors (half and bfloat16 widened exactly) or wide ``Bank``s; ``mask``: a CUDA
    ``bool`` / ``uint8`` tensor ``[nq, nt]``, packed on the device behind the current stream (``fm_mask_set_dev``), or a resident
    ``_ffi.Mask``.  (``knn`` keeps refusing a mask on wide descriptors.)  Every refusal comes before the library is touched."""
    import torch
    who = "wide_knn_masked"
    k = int(k)
    if k < 1 or k > 2:
        raise ValueError("%s: k = %d: wide float descriptors take k = 1 or 2" % (who, k))
    ops = [_wide_operand(who, x) for x in (q, t)]
    widths = [x.dim if isinstance(x, _ffi.Bank) else x.shape[1] for x in ops]
    if widths[0] != widths[1]:
        raise ValueError("%s: %d values per query row, %d per train row" % (who, widths[0], widths[1]))
    if mask is None:
        raise ValueError("%s: mask is None (knn serves wide descriptors without a mask)" % who)
    if not isinstance(mask, _ffi.Mask):
        nq, nt = (x.n if isinstance(x, _ffi.Bank) else x.shape[0] for x in ops)
        mask = _checked_mask(mask, nq, nt)
    ctx = next((x.ctx for x in ops if isinstance(x, _ffi.Bank)), None)
    made, banks = [], []
    try:
        for x in ops:
            if not isinstance(x, _ffi.Bank):
                x = bank(x, context=ctx)
                ctx = x.ctx
                made.append(x)
            banks.append(x)
        qb, tb = banks
        stream, dev = _stream_and_device(qb.ctx)
        idx = torch.empty((qb.n, k), dtype=torch.int32, device=dev)
        dist = torch.empty((qb.n, k), dtype=torch.float32, device=dev)
        mk = mask
        if not isinstance(mask, _ffi.Mask):
            mk = qb.ctx.mask(qb.n, tb.n)
            made.append(mk)
            _set_mask(mk, mask, 0)
        qb.ctx.wide_knn_masked_dev(qb, tb, mk, k, idx.data_ptr() if qb.n else 0, dist.data_ptr() if qb.n else 0, consumer_stream=stream)
        return idx, dist
    finally:
        for b in made:
            b.close()


def wide_radius_match(q, t, r, mask=None):
    """``mask`` as in ``radius_match``.
    ``cv2.BFMatcher.radiusMatch`` on wide float descriptors (129 .. 256 values per row): ``(offsets int64 [nq + 1], idx int32
    [n], dist float32 [n])`` CUDA tensors, every train row with distance < r per query row, ascending (distance, train index).
    ``q`` / ``t``: float32 / float16 / bfloat16 CUDA tensors (half and bfloat16 widened exactly) or wide ``Bank``s; ``r``: a
    scalar, or a float32 CUDA tensor [nq] read in place behind the current stream's work, as in ``radius_match`` (which keeps
    refusing wide descriptors).  One host wait for the total."""
    who = "wide_radius_match"
    ops = [_wide_operand(who, x) for x in (q, t)]
    widths = [x.dim if isinstance(x, _ffi.Bank) else x.shape[1] for x in ops]
    if widths[0] != widths[1]:
        raise ValueError("%s: %d values per query row, %d per train row" % (who, widths[0], widths[1]))
    nq = ops[0].n if isinstance(ops[0], _ffi.Bank) else ops[0].shape[0]
    ctx = next((x.ctx for x in ops if isinstance(x, _ffi.Bank)), None)
    rad, r_all = _radius(r, nq, ctx.device if ctx is not None else ops[0].device.index)
    mask = _pair_mask_checked(mask, ops[0], ops[1])
    made, banks = [], []
    try:
        for x in ops:
            if not isinstance(x, _ffi.Bank):
                x = bank(x, context=ctx)
                ctx = x.ctx
                made.append(x)
            banks.append(x)
        qb, tb = banks
        stream, dev = _stream_and_device(qb.ctx)
        if mask is not None:
            mk = _pair_mask(mask, qb, tb, made)
            return _radius_lists(lambda *a, **k: qb.ctx.radius_match_masked_dev(qb, tb, mk, *a, **k), qb.n, rad, r_all, stream, dev, False)
        return _radius_lists(lambda *a, **k: qb.ctx.wide_radius_match_dev(qb, tb, *a, **k), qb.n, rad, r_all, stream, dev, False)
    finally:
        for b in made:
            b.close()


class Collection(object):
    """A train collection fed from CUDA tensors (module docstring).  The library's collection is made with the first call
    that needs it, on ``context`` or the default context of the first tensor's device."""

    def __init__(self, context=None):
        self._context = context
        self._coll = None
        self._wide = False          # images came through add_wide: match_pairs is what the collection serves

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _refuse_wide_collection(self, who):
        """ValueError before the library is touched: a wide collection (``add_wide``) is served by ``match_pairs`` and
        ``wide_mutual_ratio_each`` only."""
        if self._wide:
            raise ValueError("Collection.%s is not built for a wide collection (images of 129 .. 256 values per row, add_wide): "
                             "match_pairs, wide_mutual_ratio_each, info and clear are" % who)

    def _collection(self, ctx=None):
        if self._coll is None:
            if self._context is None:
                self._context = ctx if ctx is not None else _ffi.default_context()
            self._coll = self._context.collection()
        return self._coll

    def add(self, tensor, *, binary=False, hamming2=False):
        """Append one image ([n, dim] uint8 / float32 / float16 / bfloat16, or ``binary`` uint8 rows of packed bits; n may be
        0), read in place behind the current stream's work -- pitched rows with unit column stride included.  Returns the
        image's index.  On return the tensor may be overwritten."""
        import torch
        self._refuse_wide_collection("add")
        if hamming2:
            raise ValueError("Collection.add: a train collection is not built for NORM_HAMMING2 (banks of that norm are matched as pairs)")
        if not binary:
            _refuse_wide("Collection.add", "a train collection (wide float images go in through add_wide)", tensor)
        tensor, dt = _checked(tensor, binary)
        coll = self._collection(_ctx_for(tensor, self._context))
        n, dim = tensor.shape
        with torch.cuda.device(tensor.device):
            stream = torch.cuda.current_stream().cuda_stream
        return coll.add_from_device(tensor.data_ptr() if n else 0, dt, n, dim, tensor.stride(0) * tensor.element_size(),
                                    stream=stream)

    def add_wide(self, tensor):
        """Append one WIDE image ([n, dim] float32 / float16 / bfloat16 with 129 <= dim <= 256; n may be 0), read in place as
        ``add`` reads its tensor (``fm_collection_add_wide_dev``).  The first ``add_wide`` makes the collection a wide one
        (``FM_BANK_F32W``): it takes no other images and serves ``match_pairs``, ``wide_mutual_ratio_each``, ``info`` and
        ``clear``.  Returns the image's index."""
        import torch
        tensor, dt = _checked(tensor)
        if dt == _ffi.FM_DT_U8:
            raise ValueError("Collection.add_wide: wide images are float32, float16 or bfloat16, got %s" % tensor.dtype)
        if not 129 <= tensor.shape[1] <= 256:
            raise ValueError("Collection.add_wide: wide images have 129 .. 256 values per row, got %d (rows of up to 128 go "
                             "to add)" % tensor.shape[1])
        if not self._wide and self.info()[0] > 0:
            raise ValueError("Collection.add_wide: the collection holds images of another kind; wide and other images do not mix")
        coll = self._collection(_ctx_for(tensor, self._context))
        n, dim = tensor.shape
        with torch.cuda.device(tensor.device):
            stream = torch.cuda.current_stream().cuda_stream
        i = coll.add_wide_from_device(tensor.data_ptr() if n else 0, dt, n, dim, tensor.stride(0) * tensor.element_size(),
                                      stream=stream)
        self._wide = True
        return i

    def _query(self, q):
        """(query bank, [banks made for this call]); every refusal before anything reaches the library."""
        self._refuse_wide_collection("knn / ratio_match / radius_match / *_each")
        _refuse_wide("Collection", "a query against a train collection", q)
        _refuse_hamming2("Collection", "a query against a train collection", q)
        if isinstance(q, _ffi.Bank):
            self._collection(q.ctx)
            return q, []
        t, _ = _checked(q)
        kind = self._collection(_ctx_for(t, self._context)).info()[3]
        b = bank(t, binary=kind == _ffi.FM_BANK_BIN, float_route=kind == _ffi.FM_BANK_F32, context=self._context)
        return b, [b]

    def mask(self, nq):
        """An all-forbidding ``_ffi.Mask`` for ``nq`` query rows on the images added so far (``Mask.set_dev`` / ``set_all`` per
        image); a later ``add`` / ``clear`` makes it stale."""
        self._refuse_wide_collection("mask")
        return self._collection().mask(nq)

    def _masks(self, masks, nq, made):
        """``masks`` as a resident Mask of the collection: one tensor per image (None: everything), checked before any is read."""
        if isinstance(masks, _ffi.Mask):
            return masks
        coll = self._collection()
        rows = coll.image_rows()
        if len(masks) != rows.shape[0]:
            raise ValueError("masks has %d entries, the collection %d images" % (len(masks), rows.shape[0]))
        checked = [None if m is None else _checked_mask(m, nq, int(rows[i]), "masks[%d]" % i) for i, m in enumerate(masks)]
        mk = coll.mask(nq)
        made.append(mk)
        for i, m in enumerate(checked):
            if m is None:
                mk.set_all(True, img=i)
            else:
                _set_mask(mk, m, i)
        return mk

    def knn(self, q, k, masks=None):
        """The k nearest rows of the stacked images: ``(img int32, idx int32, dist float32)`` [nq, k] CUDA tensors, ``idx`` the
        row inside image ``img``; ties go to the earlier image; -1 / -1 / inf beyond the collection's rows.  1 <= k <= 8.
        ``masks`` (module docstring): only the pairs they permit are candidates (``fm_collection_knn_masked_dev``)."""
        import torch
        self._refuse_wide_collection("knn")
        k = int(k)
        if k < 1:
            raise ValueError("k must be at least 1")
        qb, made = self._query(q)
        try:
            mk = self._masks(masks, qb.n, made) if masks is not None else None
            stream, dev = _stream_and_device(qb.ctx)
            img = torch.empty((qb.n, k), dtype=torch.int32, device=dev)
            idx = torch.empty((qb.n, k), dtype=torch.int32, device=dev)
            dist = torch.empty((qb.n, k), dtype=torch.float32, device=dev)
            p = (lambda t: t.data_ptr()) if qb.n else (lambda t: 0)
            if mk is None:
                self._coll.knn_dev(qb, k, p(img), p(idx), p(dist), consumer_stream=stream)
            else:
                self._coll.knn_masked_dev(qb, mk, k, p(img), p(idx), p(dist), consumer_stream=stream)
            return img, idx, dist
        finally:
            for b in made:
                b.close()

    def ratio_match(self, q, tau):
        """The classic ratio match against the stacked images: ``(qidx, img, tidx int32 [m], dist float32 [m])``, ascending
        query index.  One host wait (the count sizes the outputs)."""
        import torch
        self._refuse_wide_collection("ratio_match")
        qb, made = self._query(q)
        try:
            stream, dev = _stream_and_device(qb.ctx)
            cap = qb.n
            rows = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
            count = torch.empty(1, dtype=torch.int64, device=dev)
            m = self._coll.knn2_ratio_dev(qb, float(tau), rows.data_ptr(), count.data_ptr(), cap, want_count=True,
                                          consumer_stream=stream)
            rows = rows[:min(m, cap)]
            return (rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous(),
                    rows[:, 3].contiguous().view(torch.float32))
        finally:
            for b in made:
                b.close()

    def radius_match(self, q, r, masks=None):
        """``masks`` (one tensor per image, None = everything, or a resident Mask from ``mask``; as in ``knn``): the same lists
        without the pairs they forbid (``fm_collection_radius_match_masked_dev``).
        Every row of the stacked images with distance < r per query row: ``(offsets int64 [nq + 1], img int32 [n], idx int32
        [n], dist float32 [n])`` CUDA tensors, row i's list at ``offsets[i]:offsets[i + 1]``, ascending (distance, image, row
        inside the image).  ``r`` as in the module's ``radius_match``.  One host wait for the total."""
        self._refuse_wide_collection("radius_match")
        nq, device = _rows_and_device(q)
        rad, r_all = _radius(r, nq, device if self._context is None else self._context.device)
        qb, made = self._query(q)
        try:
            stream, dev = _stream_and_device(qb.ctx)
            coll = self._coll
            if masks is not None:
                mk = self._masks(masks, qb.n, made)
                return _radius_lists(lambda *a, **k: coll.radius_match_masked_dev(qb, mk, *a, **k), qb.n, rad, r_all, stream, dev, True)
            return _radius_lists(lambda *a, **k: coll.radius_match_dev(qb, *a, **k), qb.n, rad, r_all, stream, dev, True)
        finally:
            for b in made:
                b.close()

    def hamming_radius_match(self, q, r, masks=None):
        """``masks`` as in ``radius_match``.
        ``radius_match`` of binary descriptors against a binary collection (``add(tensor, binary=True)``): every row of the
        stacked images with ``popcount(q XOR t) < r`` per query row, ``(offsets, img, idx, dist)`` ascending (h, image, row
        inside the image).  ``q``: a uint8 CUDA tensor of packed bits or a binary ``Bank``; ``r`` as in the module's
        ``radius_match``.  One host wait for the total."""
        self._refuse_wide_collection("hamming_radius_match")
        x = _binary_operand("Collection.hamming_radius_match", q)
        is_bank = isinstance(x, _ffi.Bank)
        nq, device = (x.n, x.ctx.device) if is_bank else (x.shape[0], x.device.index)
        rad, r_all = _radius(r, nq, device if self._context is None else self._context.device)
        coll = self._collection(x.ctx if is_bank else _ctx_for(x, self._context))
        qb = x if is_bank else bank(x, binary=True, context=self._context)
        made = [] if is_bank else [qb]
        try:
            stream, dev = _stream_and_device(qb.ctx)
            if masks is not None:
                mk = self._masks(masks, qb.n, made)
                return _radius_lists(lambda *a, **k: coll.radius_match_masked_dev(qb, mk, *a, **k), qb.n, rad, r_all, stream, dev, True)
            return _radius_lists(lambda *a, **k: coll.hamming_radius_match_dev(qb, *a, **k), qb.n, rad, r_all, stream, dev, True)
        finally:
            for b in made:
                b.close()

    def fast_match_each(self, q, tau, cap=None):
        """Fast-Match's accepted-match test of ``q`` inside every image separately, left on the device: ``(rows int32
        [n_images, cap, 3] = (query, row inside the image, float32 distance bits), counts int64 [n_images] = min(accepted,
        cap))``; ``cap`` defaults to ``q.n``.  ``q`` is a ``Bank`` that carries self distances; enqueued, no host wait."""
        import torch
        self._refuse_wide_collection("fast_match_each")
        if not isinstance(q, _ffi.Bank):
            raise ValueError("fast_match_each takes a resident Bank that carries self distances (Context.self_dist_batch)")
        coll = self._collection(q.ctx)
        ni = coll.info()[0]
        cap = q.n if cap is None else int(cap)
        stream, dev = _stream_and_device(q.ctx)
        rows = torch.empty((ni, max(cap, 0), 3), dtype=torch.int32, device=dev)
        counts = torch.zeros(ni, dtype=torch.int64, device=dev)
        coll.match_accepted_each_dev(q, float(tau), rows.data_ptr() if rows.numel() else 0, counts.data_ptr() if ni else 0, cap,
                                     consumer_stream=stream)
        return rows, counts

    def hamming_fast_match_each(self, q, tau, cap=None):
        """``fast_match_each`` on a binary collection (``add(tensor, binary=True)``): ``q`` is a binary ``Bank`` that carries
        Hamming self distances (``Context.hamming_self_dist_batch``); ``(rows, counts)`` as there, the distance bits those of
        popcount(q XOR t); enqueued, no host wait."""
        import torch
        self._refuse_wide_collection("hamming_fast_match_each")
        if not isinstance(q, _ffi.Bank) or q.kind != _ffi.FM_BANK_BIN:
            raise ValueError("hamming_fast_match_each takes a resident binary Bank that carries Hamming self distances "
                             "(Context.hamming_self_dist_batch); fast_match_each is the L2 call")
        coll = self._collection(q.ctx)
        ni = coll.info()[0]
        cap = q.n if cap is None else int(cap)
        stream, dev = _stream_and_device(q.ctx)
        rows = torch.empty((ni, max(cap, 0), 3), dtype=torch.int32, device=dev)
        counts = torch.zeros(ni, dtype=torch.int64, device=dev)
        coll.hamming_match_accepted_each_dev(q, float(tau), rows.data_ptr() if rows.numel() else 0, counts.data_ptr() if ni else 0,
                                             cap, consumer_stream=stream)
        return rows, counts

    def mutual_nn_each(self, q, max_dist=None, cap=None):
        """Mutual nearest neighbours of ``q`` inside every image separately, left on the device: ``(rows int32 [n_images, cap,
        3] = (query, row inside the image, float32 distance bits), counts int64 [n_images] = min(matched, cap))``, rows
        ascending in query index; ``cap`` defaults to the query's rows.  A match is kept while ``dist < max_dist`` (strict
        float32 compare; None: every match).  ``q`` is a ``Bank`` or a CUDA tensor as ``add`` takes them (packed bits for a
        binary collection).  Enqueued, no host wait."""
        import torch
        self._refuse_wide_collection("mutual_nn_each")
        if cap is not None and int(cap) < 0:
            raise ValueError("cap must not be negative")
        max_dist = float("inf") if max_dist is None else float(np.float32(max_dist))
        qb, made = self._query(q)
        try:
            ni = self._coll.info()[0]
            cap = qb.n if cap is None else int(cap)
            stream, dev = _stream_and_device(qb.ctx)
            rows = torch.empty((ni, cap, 3), dtype=torch.int32, device=dev)
            counts = torch.zeros(ni, dtype=torch.int64, device=dev)
            self._coll.xcheck1_each_dev(qb, max_dist, rows.data_ptr() if rows.numel() else 0, counts.data_ptr() if ni else 0, cap,
                                        consumer_stream=stream)
            return rows, counts
        finally:
            for b in made:
                b.close()

    def mutual_ratio_each(self, q, tau, symmetric=False, cap=None):
        """``mutual_ratio_match`` of ``q`` inside every image separately, left on the device: ``(rows int32 [n_images, cap, 3] =
        (query, row inside the image, float32 distance bits), counts int64 [n_images] = min(accepted, cap))``, rows ascending
        in query index; ``cap`` defaults to the query's rows.  ``q`` is a ``Bank`` or a CUDA tensor as ``add`` takes them.  One
        host wait inside the library (the candidate count)."""
        import torch
        self._refuse_wide_collection("mutual_ratio_each")
        if cap is not None and int(cap) < 0:
            raise ValueError("cap must not be negative")
        qb, made = self._query(q)
        try:
            ni = self._coll.info()[0]
            cap = qb.n if cap is None else int(cap)
            stream, dev = _stream_and_device(qb.ctx)
            rows = torch.empty((ni, cap, 3), dtype=torch.int32, device=dev)
            counts = torch.zeros(ni, dtype=torch.int64, device=dev)
            self._coll.mutual_ratio_each_dev(qb, float(tau), bool(symmetric), rows.data_ptr() if rows.numel() else 0,
                                             counts.data_ptr() if ni else 0, cap, consumer_stream=stream)
            return rows, counts
        finally:
            for b in made:
                b.close()

    def match_pairs(self, pairs=None, tau=0.8, symmetric=False, cap=None):
        """The images of the collection matched against each other (the match graph), left on the device: ``(offsets int64
        [n_pairs + 1], rows int32 [n, 3] = (row in image a, row in image b, float32 distance bits))``; the rows of pair p =
        (a, b) are ``rows[offsets[p]:offsets[p + 1]]``, equal to ``mutual_ratio_match(image_a, image_b, tau, symmetric)``.
        ``pairs``: a host sequence of ordered (a, b) image indices or an int32 CPU tensor [n_pairs, 2]; None: every a < b in
        lexicographic order.  ``cap`` rows are allocated and the longest prefix of whole pairs that fits is written (the
        offsets always hold the full counts); enqueued, no host wait.  ``cap`` None: a counts-only call first, whose total
        is read back (the one host wait), then one fill of exactly that size."""
        import torch
        if cap is not None and int(cap) < 0:
            raise ValueError("cap must not be negative")
        if pairs is not None:
            if torch.is_tensor(pairs):
                if pairs.is_cuda or pairs.dtype != torch.int32:
                    raise ValueError("pairs must be a host sequence or an int32 CPU tensor [n_pairs, 2]")
                pairs = pairs.contiguous().numpy()
            pairs = _ffi.pairs_array(pairs, self.info()[0])
        coll = self._collection()
        n = coll.info()[0] * (coll.info()[0] - 1) // 2 if pairs is None else pairs.shape[0]
        stream, dev = _stream_and_device(coll.ctx)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if cap is None:
            cap = coll.pairs_mutual_ratio_dev(pairs, float(tau), bool(symmetric), offsets.data_ptr(), 0, 0, want_total=True,
                                              consumer_stream=stream)
        cap = int(cap)
        rows = torch.empty((cap, 3), dtype=torch.int32, device=dev)
        coll.pairs_mutual_ratio_dev(pairs, float(tau), bool(symmetric), offsets.data_ptr(), rows.data_ptr() if cap else 0, cap,
                                    consumer_stream=stream)
        return offsets, rows

    def wide_mutual_ratio_each(self, q, tau, symmetric=False, cap=None):
        """A wide query matched against every image of a WIDE collection (``add_wide``), image by image, left on the device:
        ``(offsets int64 [n_images + 1], rows int32 [n, 3] = (query row, row inside the image, float32 distance bits))``; the
        rows of image i are ``rows[offsets[i]:offsets[i + 1]]``, equal to ``mutual_ratio_match(q, image_i, tau, symmetric)``.
        ``q``: a wide ``Bank`` or a CUDA tensor [nq, dim] of float32 / float16 / bfloat16 with 129 <= dim <= 256.  ``cap``
        exactly as in ``match_pairs``.  ``ValueError`` before the library is touched for a collection that is not wide."""
        import torch
        if not self._wide:
            raise ValueError("Collection.wide_mutual_ratio_each: the collection is not a wide one (add_wide); "
                             "mutual_ratio_each serves the other kinds")
        if cap is not None and int(cap) < 0:
            raise ValueError("cap must not be negative")
        made = []
        if isinstance(q, _ffi.Bank):
            if q.kind != _ffi.FM_BANK_F32W:
                raise ValueError("Collection.wide_mutual_ratio_each: the query bank is not a wide float bank (FM_BANK_F32W)")
            qb = q
        else:
            t, dt = _checked(q)
            if dt == _ffi.FM_DT_U8 or not 129 <= t.shape[1] <= 256:
                raise ValueError("Collection.wide_mutual_ratio_each: the query is a float32 / float16 / bfloat16 tensor of "
                                 "129 .. 256 values per row, got %s [%d, %d]" % (t.dtype, t.shape[0], t.shape[1]))
            qb = bank(t, context=self._context)
            made.append(qb)
        try:
            coll = self._collection(qb.ctx)
            n = coll.info()[0]
            stream, dev = _stream_and_device(coll.ctx)
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
            if cap is None:
                cap = coll.wide_mutual_ratio_each_dev(qb, float(tau), bool(symmetric), offsets.data_ptr(), 0, 0, want_total=True,
                                                      consumer_stream=stream)
            cap = int(cap)
            rows = torch.empty((cap, 3), dtype=torch.int32, device=dev)
            coll.wide_mutual_ratio_each_dev(qb, float(tau), bool(symmetric), offsets.data_ptr(), rows.data_ptr() if cap else 0, cap,
                                            consumer_stream=stream)
            return offsets, rows
        finally:
            for b in made:
                b.close()

    def wide_fast_match_each(self, q, tau, cap=None):
        """``fast_match_each`` on a WIDE collection (``add_wide``): Fast-Match's accepted-match test of a wide query inside
        every image separately, left on the device -- ``(rows int32 [n_images, cap, 3] = (query, row inside the image, float32
        distance bits), counts int64 [n_images] = min(accepted, cap))``, image i equal to ``wide_fast_match(q, image_i, tau)``;
        ``cap`` defaults to the query's rows.  ``q``: a wide ``Bank`` or a CUDA tensor [nq, dim] of float32 / float16 /
        bfloat16; self distances it does not carry are computed on the device (``fm_wide_self_dist_batch``).  Enqueued, no host
        wait.  ``ValueError`` before the library is touched for a collection that is not wide."""
        import torch
        if not self._wide:
            raise ValueError("Collection.wide_fast_match_each: the collection is not a wide one (add_wide); "
                             "fast_match_each / hamming_fast_match_each serve the other kinds")
        if cap is not None and int(cap) < 0:
            raise ValueError("cap must not be negative")
        x = _wide_operand("Collection.wide_fast_match_each", q)
        made = []
        qb = x
        if not isinstance(x, _ffi.Bank):
            qb = bank(x, context=self._context)
            made.append(qb)
        try:
            coll = self._collection(qb.ctx)
            if not qb.has_selfdist:
                qb.ctx.wide_self_dist_batch([qb], want_host=False)
            ni = coll.info()[0]
            cap = qb.n if cap is None else int(cap)
            stream, dev = _stream_and_device(qb.ctx)
            rows = torch.empty((ni, max(cap, 0), 3), dtype=torch.int32, device=dev)
            counts = torch.zeros(ni, dtype=torch.int64, device=dev)
            coll.wide_match_accepted_each_dev(qb, float(tau), rows.data_ptr() if rows.numel() else 0, counts.data_ptr() if ni else 0,
                                              cap, consumer_stream=stream)
            return rows, counts
        finally:
            for b in made:
                b.close()

    def wide_radius_match(self, q, r):
        """``radius_match`` on a WIDE collection (``add_wide``): every row of the stacked images with distance < r per query
        row, ``(offsets int64 [nq + 1], img int32 [n], idx int32 [n], dist float32 [n])`` CUDA tensors, ascending (distance,
        image, row inside the image).  ``q``: a wide ``Bank`` or a CUDA tensor [nq, dim] of float32 / float16 / bfloat16 with
        129 <= dim <= 256; ``r`` as in the module's ``radius_match``.  One host wait for the total.  ``ValueError`` before the
        library is touched for a collection that is not wide."""
        if not self._wide:
            raise ValueError("Collection.wide_radius_match: the collection is not a wide one (add_wide); "
                             "radius_match / hamming_radius_match serve the other kinds")
        x = _wide_operand("Collection.wide_radius_match", q)
        is_bank = isinstance(x, _ffi.Bank)
        nq, device = (x.n, x.ctx.device) if is_bank else (x.shape[0], x.device.index)
        rad, r_all = _radius(r, nq, device if self._context is None else self._context.device)
        coll = self._collection(x.ctx if is_bank else _ctx_for(x, self._context))
        qb = x if is_bank else bank(x, context=self._context)
        try:
            stream, dev = _stream_and_device(qb.ctx)
            return _radius_lists(lambda *a, **k: coll.wide_radius_match_dev(qb, *a, **k), qb.n, rad, r_all, stream, dev, True)
        finally:
            if not is_bank:
                qb.close()

    def _wide_stacked_query(self, who, q):
        """The query bank of a wide stacked call and the banks made for it -- ``ValueError`` before the library is touched for a
        collection that is not wide and for a query that is not a wide operand."""
        if not self._wide:
            raise ValueError("Collection.%s: the collection is not a wide one (add_wide); knn / ratio_match serve the other "
                             "kinds" % who)
        x = _wide_operand("Collection.%s" % who, q)
        if isinstance(x, _ffi.Bank):
            return x, []
        qb = bank(x, context=self._context)
        return qb, [qb]

    def wide_knn(self, q, k):
        """``knn`` on a WIDE collection (``add_wide``): the k nearest rows of ALL images' stacked rows, ``(img int32, idx int32,
        dist float32)`` [nq, k] CUDA tensors shaped like ``knn``'s -- ``knn(q, the images' rows concatenated, k)`` with every
        hit located; -1 / -1 / inf beyond the collection's rows.  k = 1, 2.  ``q``: a wide ``Bank`` or a CUDA tensor [nq, dim]
        of float32 / float16 / bfloat16 with 129 <= dim <= 256.  Enqueued, no host wait (``fm_collection_wide_knn_dev``).
        ``ValueError`` before the library is touched for a collection that is not wide and for k outside 1, 2."""
        import torch
        k = int(k)
        if k < 1 or k > 2:
            raise ValueError("Collection.wide_knn: k = %d: wide float descriptors get k-NN lists for k = 1, 2" % k)
        qb, made = self._wide_stacked_query("wide_knn", q)
        try:
            coll = self._collection(qb.ctx)
            stream, dev = _stream_and_device(qb.ctx)
            img = torch.empty((qb.n, k), dtype=torch.int32, device=dev)
            idx = torch.empty((qb.n, k), dtype=torch.int32, device=dev)
            dist = torch.empty((qb.n, k), dtype=torch.float32, device=dev)
            p = (lambda t: t.data_ptr()) if qb.n else (lambda t: 0)
            coll.wide_knn_dev(qb, k, p(img), p(idx), p(dist), consumer_stream=stream)
            return img, idx, dist
        finally:
            for b in made:
                b.close()

    def wide_ratio_match(self, q, tau):
        """``ratio_match`` on a WIDE collection: Lowe's test on the 2-NN lists over ALL images' rows, ``(qidx, img, tidx int32
        [m], dist float32 [m])``, ascending query index (``fm_collection_wide_knn2_ratio_dev``).  ``q`` as in ``wide_knn``.
        One host wait (the count sizes the outputs)."""
        import torch
        qb, made = self._wide_stacked_query("wide_ratio_match", q)
        try:
            coll = self._collection(qb.ctx)
            stream, dev = _stream_and_device(qb.ctx)
            cap = qb.n
            rows = torch.empty((max(cap, 1), 4), dtype=torch.int32, device=dev)
            count = torch.empty(1, dtype=torch.int64, device=dev)
            m = coll.wide_knn2_ratio_dev(qb, float(tau), rows.data_ptr(), count.data_ptr(), cap, want_count=True,
                                         consumer_stream=stream)
            rows = rows[:min(m, cap)]
            return (rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous(),
                    rows[:, 3].contiguous().view(torch.float32))
        finally:
            for b in made:
                b.close()

    def wide_votes(self, q, tau, mode=0):
        """Query rows that pass the ratio test d0 / d1 < tau per image of a WIDE collection: an int64 [n_images] CUDA tensor
        (mode 0: the test on the lists over all images, counted at the first neighbour's image; 1: on every image's own 2-NN
        lists).  ``q`` as in ``wide_knn``.  The library counts on the device and hands the counts to the host
        (``fm_collection_wide_votes``); they are put back on the query's device: one host wait."""
        import torch
        if mode not in (0, 1):
            raise ValueError("Collection.wide_votes: mode must be 0 (stacked lists) or 1 (per-image lists)")
        qb, made = self._wide_stacked_query("wide_votes", q)
        try:
            coll = self._collection(qb.ctx)
            _, dev = _stream_and_device(qb.ctx)
            # (a host-form call: the query's rows must be there when it runs on the context's stream)
            with torch.cuda.device(dev):
                torch.cuda.current_stream().synchronize()
            return torch.from_numpy(coll.wide_votes(qb, float(tau), int(mode))).to(dev)
        finally:
            for b in made:
                b.close()

    def clear(self):
        if self._coll is not None:
            self._coll.clear()
        self._wide = False

    def info(self):
        """(n_images, n_rows_total, dim, kind)"""
        return self._coll.info() if self._coll is not None else (0, 0, 0, 0)

    def close(self):
        if self._coll is not None:
            self._coll.close()
        self._coll = None
