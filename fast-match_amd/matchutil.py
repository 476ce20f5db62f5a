"""Matcher wrappers with the reference's operator signatures, running on the HIP path.

Mirrors ``matchutil.py`` of the reference:

* ``bf_match(dt1, dt2, k=1, options={})``     -- reference ``matchutil.py:39-43``
  (``cv2.BFMatcher(cv2.NORM_L2, crossCheck).knnMatch(dt1, dt2, k=k)``; crossCheck is
  honoured only when ``k == 1``).
* ``flann_match(dt1, dt2, k=1, options={})``  -- reference ``matchutil.py:46-67``.  The
  reference's FLANN index is randomized and approximate; the exact brute-force k-NN it
  approximates is returned instead, so results are
  deterministic.
* ``bf_radius_match(dt1, dt2, maxDistance, options={})`` -- ``cv2.BFMatcher(cv2.NORM_L2)
  .radiusMatch(dt1, dt2, maxDistance)`` (compactResult False; the reference has no call
  site): every train row with distance < maxDistance, one list per query row ascending
  by (distance, train index).  ``maxDistance`` may also be one radius per query row.
* ``hamming_radius_match(dt1, dt2, maxDistance, options={})`` / ``hamming_radius_match_arrays`` --
  ``cv2.BFMatcher(cv2.NORM_HAMMING).radiusMatch`` on binary descriptors (uint8 rows of 1 .. 64 bytes, or resident binary
  banks): every train row with ``popcount(q XOR t) < maxDistance`` (strict, float32: ``h <= H`` is ``H + 0.5``), one list
  per query row ascending by (h, train index) (``fm_hamming_radius_match``).  ``bf_radius_match`` stays the NORM_L2 call.
* ``hamming_fast_match(dt1, dt2, tau, options={})`` / ``hamming_fast_match_arrays`` -- Fast-Match's accepted-match test on
  binary descriptors: the cross-checked nearest neighbour t of q under ``popcount(q XOR t)`` is accepted iff
  ``dist / selfdist(q) < tau``, ``selfdist(q)`` the Hamming distance from q to its nearest OTHER row of ``dt1``
  (``fm_hamming_self_dist_batch``, ``fm_hamming_match_accepted``).  Against a collection, image by image:
  ``BFMatcher(NORM_HAMMING).hammingFastMatchEach`` / ``hammingFastMatchEach_arrays``; ``fastMatchEach`` stays the NORM_L2 call.
* ``options["normType"]``: ``NORM_L2`` (4, the default) or ``NORM_HAMMING`` (6) -- cv2's values.  With
  ``NORM_HAMMING`` the descriptors are binary (ORB, BRIEF, BRISK, FREAK, AKAZE: uint8 rows of 1 .. 64 bytes,
  ``Context.bank_binary``) and the distance is the bit count of ``q XOR t`` (``cv2.BFMatcher(cv2.NORM_HAMMING,
  crossCheck)``); ``bf_match``, ``flann_match`` and ``ratio_match_arrays`` honour it, ``bf_radius_match`` does not
  (``ValueError``: ``hamming_radius_match`` is the call), nor does anything else take ``NORM_HAMMING2``.  Without ``normType`` every array is an L2 bank,
  a uint8 [n, 32] array included.
* ``NORM_HAMMING2`` (7; ORB with ``WTA_K`` = 3 or 4, every descriptor element a 2-bit value) has calls of its own:
  ``hamming2_match`` / ``hamming2_match_arrays`` (knnMatch, 1 <= k <= 8, crossCheck at k == 1), ``hamming2_ratio_match_arrays``,
  ``hamming2_mutual_ratio_match_arrays``, ``hamming2_radius_match`` / ``hamming2_radius_match_arrays`` and cv2's factory
  ``BFMatcher_create(7)``, whose object takes ``match`` / ``knnMatch`` / ``radiusMatch`` with a train argument.  The distance is
  the number of 2-bit cells (bits 2c, 2c + 1 of a byte) in which two rows differ.  On the matrix cores a cell (a, b) is three
  FP4 values (s_a, s_b, s_a s_b), s = +-1 -- the vertices of a tetrahedron -- so the dot product of two rows of P = 4 bytes
  cells is 3 P - 4 h2, exact in float32 (``csrc/hamming2.hip``; 12 bytes values per row, ceil(12 bytes / 128) K steps: 1 .. 10
  bytes one, .. 21 two, .. 32 three, .. 42 four, .. 53 five, .. 64 six; the sweeps hold two 128-row stages in 20,480 ..
  102,400 bytes of LDS and 224 .. 400 registers, no scratch: DESIGN.md, K11b, which also has the measured cost beside
  NORM_HAMMING -- 1.14 x to 1.28 x on the same rows).  Served by the library for two such banks: ``fm_knn2``, ``fm_knn``,
  ``fm_xcheck1``, ``fm_knn2_ratio``, ``fm_mutual_ratio``, their ``_dev`` forms, ``fm_hamming_radius_match(_dev)``; every other
  entry point refuses them (``FM_EUNSUPPORTED``).  Not built for this norm, ``ValueError`` before
  anything is uploaded: ``options["normType"] = 7`` in the other calls, ``BFMatcher(7)``, masks, train collections
  (``add`` / ``train`` / a call without a train argument), Fast-Match's self-distance test.
* Wide float descriptors -- float arrays of 129 .. 256 values per row, SuperPoint's 256-D rows for one -- go to the
  library's wide float banks under ``NORM_L2``: ``bf_match`` with k <= 2 and with crossCheck, ``ratio_match_arrays`` and
  ``mutual_ratio_match_arrays`` take them; ``bf_radius_match``, a mask, k >= 3 and ``BFMatcher.add`` raise ``ValueError``
  before anything is uploaded.  ``BFMatcher.add_wide`` adds wide images to a collection of their own, whose match graph
  ``matchPairs`` / ``matchPairs_arrays`` computes (``fm_collection_add_wide``).  A wide query against such a collection,
  image by image, is ``BFMatcher.mutualRatioMatchWideEach`` / ``mutualRatioMatchWideEach_arrays`` (mutual nearest neighbour
  + ratio per image, the visual-localisation pattern; ``fm_collection_wide_mutual_ratio_each``) and
  ``knnMatchWideEach_arrays`` (``fm_collection_wide_knn2_each``).  Fast-Match's self-distance test on wide descriptors:
  ``wide_fast_match`` / ``wide_fast_match_arrays`` (``fm_wide_self_dist_batch``, ``fm_wide_match_accepted``) and, against a
  wide collection, ``BFMatcher.wideFastMatchEach`` / ``wideFastMatchEach_arrays``.  knnMatch under a mask on wide descriptors
  (guided matching: a window round a predicted position, an epipolar band) is ``wide_bf_match_masked`` /
  ``wide_bf_match_masked_arrays`` (``fm_wide_knn_masked``, k = 1 or 2); ``bf_match`` keeps refusing the combination.
* radiusMatch under a mask (guided matching: every row within r among the rows of a window or an epipolar band):
  ``bf_radius_match_masked`` / ``bf_radius_match_masked_arrays`` (``fm_radius_match_masked``: uint8 and float 128-D rows,
  NORM_HAMMING rows, wide float rows -- the masked threshold sweeps on the matrix cores), and
  ``BFMatcher.radiusMatch(query, train, maxDistance, mask=None, compactResult=False)``.  ``bf_radius_match`` keeps refusing
  ``options["mask"]``.
* ``options["mask"]``: cv2's ``mask`` argument of ``knnMatch`` -- an ``[nq, nt]`` uint8 / bool array, nonzero = the pair
  (query row, train row) may be matched, or a resident ``_ffi.Mask`` (``Context.mask``).  ``bf_match``,
  ``bf_match_arrays``, ``flann_match`` and ``flann_match_arrays`` honour it when crossCheck is off: every list is the
  unmasked list computed over the permitted train rows only (``fm_knn_masked``; -1 / inf, or a shorter DMatch list, where
  fewer than k rows are permitted).  Its shape is checked before anything is uploaded.  ``ValueError`` naming what is not
  built: a mask with crossCheck, in ``bf_radius_match``, ``ratio_match_arrays`` and ``mutual_ratio_match_arrays``.
  ``BFMatcher.knnMatch(query, train=None, k=None, mask=None, masks=None)`` and ``match`` take cv2's keywords: ``mask`` with a
  train argument, ``masks`` (one entry per added image, ``None`` = everything permitted) against the collection
  (``fm_collection_knn_masked``).  Calls without a mask go exactly where they went before masks existed.
* ``BFMatcher(normType, crossCheck)`` -- cv2's matcher object: ``add`` / ``train`` / ``clear`` build a TRAIN COLLECTION and
  ``match(query)`` / ``knnMatch(query, k)`` search all of its images at once, filling ``DMatch.imgIdx`` (``fm_collection_*``).
* ``sift / get_features / get_keypoints``     -- reference ``matchutil.py:22-36``; SIFT
  stays in OpenCV on the host and needs ``cv2``.

The return value is the same shape OpenCV gives: a list with one inner list per query
row holding up to ``k`` ``DMatch`` objects (any number for ``bf_radius_match``) (attributes ``queryIdx, trainIdx, imgIdx,
distance``).  ``*_arrays`` variants return NumPy arrays and skip the Python objects.
Errors (dtype/width mismatch, unsupported k) raise ``FastMatchHipError``/``ValueError``
where cv2 would raise ``cv2.error``.  There is no CPU fallback.
"""
import numpy as np

from . import _ffi

NORM_L2 = 4             # cv2.NORM_L2
NORM_HAMMING = 6        # cv2.NORM_HAMMING
NORM_HAMMING2 = 7       # cv2.NORM_HAMMING2 (ORB with WTA_K = 3 or 4): served by the hamming2_* calls and BFMatcher_create(7)


class DMatch(object):
    """Stand-in for cv2.DMatch (same attribute names)."""
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx, trainIdx, distance, imgIdx=0):
        self.queryIdx = int(queryIdx)
        self.trainIdx = int(trainIdx)
        self.imgIdx = int(imgIdx)
        self.distance = float(distance)

    def __repr__(self):
        return "DMatch(queryIdx=%d, trainIdx=%d, distance=%r)" % (self.queryIdx, self.trainIdx, self.distance)


def _context(options):
    ctx = options.get("context") if options else None
    if ctx is not None:
        return ctx
    return _ffi.default_context(options.get("device") if options else None)


def _as_bank(ctx, d):
    """Accept a resident Bank or an ndarray (uploaded for this call only)."""
    if isinstance(d, _ffi.Bank):
        return d, False
    a = np.asarray(d)
    if a.ndim != 2:
        raise ValueError("descriptors must be a 2-D [n, dim] array")
    return ctx.bank(a), True


def _norm_type(options, dt1, dt2):
    """options["normType"], checked against the operands BEFORE anything is uploaded (cv2 asserts the same in its matcher)."""
    norm = options.get("normType", NORM_L2) if options else NORM_L2
    if norm not in (NORM_L2, NORM_HAMMING):
        raise ValueError("normType %r: this call takes NORM_L2 (4) and NORM_HAMMING (6) only%s"
                         % (norm, " (NORM_HAMMING2 is served by hamming2_match, hamming2_match_arrays, hamming2_ratio_match_arrays, "
                                  "hamming2_mutual_ratio_match_arrays, hamming2_radius_match and BFMatcher_create(7))" if norm == 7 else ""))
    for d in (dt1, dt2):
        if isinstance(d, _ffi.Bank) and d.kind == _ffi.FM_BANK_BIN2:
            raise ValueError("a NORM_HAMMING2 bank (Context.bank_binary2) goes with the hamming2_* calls and BFMatcher_create(7) only")
        if isinstance(d, _ffi.Bank):
            if (d.kind == _ffi.FM_BANK_BIN) != (norm == NORM_HAMMING):
                raise ValueError("a binary bank (Context.bank_binary) goes with normType NORM_HAMMING, and only it"
                                 if d.kind == _ffi.FM_BANK_BIN else "NORM_HAMMING needs binary banks (Context.bank_binary)")
        elif norm == NORM_HAMMING and np.asarray(d).dtype != np.uint8:
            raise ValueError("NORM_HAMMING needs uint8 descriptors (cv2 asserts CV_8U), got %s" % np.asarray(d).dtype)
    return norm


def _bank_pair(ctx, dt1, dt2, norm):
    if norm != NORM_HAMMING:
        return _as_bank_pair(ctx, dt1, dt2)
    banks = []
    try:
        for d in (dt1, dt2):
            banks.append((d, False) if isinstance(d, _ffi.Bank) else (ctx.bank_binary(np.asarray(d)), True))
    except Exception:
        for b, tmp in banks:
            if tmp:
                b.close()
        raise
    return banks[0][0], banks[0][1], banks[1][0], banks[1][1]


def _as_bank_pair(ctx, dt1, dt2):
    """Both operands as banks of ONE kind.  A float32 array whose values all happen to be
    integers in 0..255 is uploaded on the exact int8 route, any other float32 array on the
    float32 route; cv2.BFMatcher takes any two float32 arrays, so when the two kinds differ
    (say a one-row all-zero bank against normalised descriptors) the integer-valued array is
    uploaded again on the float32 route, which yields the same numbers for it.  A resident
    Bank of the other kind cannot be re-uploaded: the library then reports the mismatch."""
    qb, q_tmp = _as_bank(ctx, dt1)
    try:
        tb, t_tmp = _as_bank(ctx, dt2)
    except Exception:
        if q_tmp:
            qb.close()
        raise
    if qb.kind != tb.kind:
        if q_tmp and qb.kind == _ffi.FM_BANK_I8 and np.asarray(dt1).dtype != np.uint8:
            qb.close()
            qb = ctx.bank(np.asarray(dt1), float_route=True)
        elif t_tmp and tb.kind == _ffi.FM_BANK_I8 and np.asarray(dt2).dtype != np.uint8:
            tb.close()
            tb = ctx.bank(np.asarray(dt2), float_route=True)
    return qb, q_tmp, tb, t_tmp


def _rows_of(d):
    return d.n if isinstance(d, _ffi.Bank) else np.asarray(d).shape[0]


def _is_wide(d):
    """A wide float operand: a resident FM_BANK_F32W bank, or a float array of more than 128 columns."""
    if isinstance(d, _ffi.Bank):
        return d.kind == _ffi.FM_BANK_F32W
    a = np.asarray(d)
    return a.ndim == 2 and a.shape[1] > 128 and a.dtype != np.uint8


def _refuse_wide(who, what, *operands):
    """ValueError BEFORE anything is uploaded: wide float descriptors (129 .. 256 values per row) are served by knnMatch with
    k <= 2, crossCheck, the ratio match and the mutual ratio match only."""
    if any(_is_wide(d) for d in operands):
        raise ValueError("%s: %s is not built for wide float descriptors (129 .. 256 values per row: k <= 2, crossCheck, "
                         "ratio_match_arrays and mutual_ratio_match_arrays are)" % (who, what))


def _mask_array(m, nq, nt, what):
    """A host mask as a uint8 [nq, nt] array, or ValueError."""
    a = np.asarray(m)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    if a.dtype != np.uint8:
        raise ValueError("%s must be uint8 or bool (cv2 asserts CV_8U), got %s" % (what, a.dtype))
    if a.ndim != 2 or a.shape != (nq, nt):
        raise ValueError("%s must be [%d, %d] (query rows, train rows), got %s" % (what, nq, nt, a.shape))
    return a


def _mask_option(options, dt1, dt2, who, not_built=None):
    """options["mask"] checked against the operands BEFORE anything is uploaded: None, a resident Mask, or a uint8 array.
    not_built: what the caller would have to honour it in -- a ValueError that names it."""
    m = options.get("mask") if options else None
    if m is None:
        return None
    if not_built:
        raise ValueError("%s: a mask with %s is not built (masks are honoured by knnMatch / match without crossCheck: "
                         "bf_match, flann_match, BFMatcher.knnMatch)" % (who, not_built))
    nq, nt = _rows_of(dt1), _rows_of(dt2)
    if isinstance(m, _ffi.Mask):
        if m.n_images != 0 or (m.nq, m.nt) != (nq, nt):
            raise ValueError("%s: the Mask is for %d x %d rows%s, the operands have %d x %d"
                             % (who, m.nq, m.nt, " of a collection" if m.n_images else "", nq, nt))
        return m
    return _mask_array(m, nq, nt, "%s: options['mask']" % who)


def bf_match_arrays(dt1, dt2, k=1, options={}):
    """Array form of :func:`bf_match`.

    crossCheck (k == 1 only): returns ``(tidx int32[nq], dist float32[nq])`` with
    ``tidx == -1`` where OpenCV returns an empty inner list.
    Otherwise returns ``(idx int32[nq, k], dist float32[nq, k])`` with ``-1`` / ``inf``
    where the train set has fewer than k rows (1 <= k <= 8; ``matchutil.py:39-43`` passes any k to cv2)."""
    k = int(k)
    if k < 1:
        raise ValueError("bf_match: k must be at least 1")
    if k > 8:
        # cv2.BFMatcher.knnMatch takes any k; the reference calls k = 1 and 2 (fastmatch.pyx:122-123, 161-162, cache.pyx:250)
        raise ValueError("bf_match: k = %d: the HIP path builds k-NN lists up to k = 8 (FM_EUNSUPPORTED beyond)" % k)
    crossCheck = k == 1 and options.get("crossCheck", False) == True   # noqa: E712  (reference semantics)
    norm = _norm_type(options, dt1, dt2)
    mask = _mask_option(options, dt1, dt2, "bf_match", "crossCheck" if crossCheck else None)
    if mask is not None:
        _refuse_wide("bf_match", "a mask", dt1, dt2)
    if k > 2:
        _refuse_wide("bf_match", "k >= 3", dt1, dt2)
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _bank_pair(ctx, dt1, dt2, norm)
    try:
        if mask is not None:
            if isinstance(mask, _ffi.Mask):
                return ctx.knn_masked(qb, tb, mask, k)
            with ctx.mask(qb.n, tb.n) as mk:
                return ctx.knn_masked(qb, tb, mk.set(mask), k)
        if crossCheck:
            return ctx.xcheck1(qb, tb)
        if k > 2:
            return ctx.knn(qb, tb, k)                   # exact lists off the matrix cores (fm_knn)
        idx, dist = ctx.knn2(qb, tb)
        return idx[:, :k], dist[:, :k]
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def matches_from_arrays(idx, dist):
    """Build OpenCV's list-of-lists of DMatch from index/distance arrays."""
    idx = np.asarray(idx)
    dist = np.asarray(dist)
    if idx.ndim == 1:
        idx = idx[:, None]
        dist = dist[:, None]
    out = []
    for qi in range(idx.shape[0]):
        row = [DMatch(qi, idx[qi, j], dist[qi, j]) for j in range(idx.shape[1]) if idx[qi, j] >= 0]
        out.append(row)
    return out


def bf_match(dt1, dt2, k=1, options={}):
    """ Use the HIP brute-force matcher with OpenCV BFMatcher(normType) semantics (NORM_L2 unless options say NORM_HAMMING) """
    idx, dist = bf_match_arrays(dt1, dt2, k=k, options=options)
    return matches_from_arrays(idx, dist)


def flann_match(dt1, dt2, k=1, options={}):
    """ Exact k-NN in place of the reference's approximate FLANN kd-tree search.
    ``algorithm`` / ``trees`` / ``checks`` are accepted and ignored. """
    opts = dict(options)
    opts.pop("crossCheck", None)
    return bf_match(dt1, dt2, k=k, options=opts)


def flann_match_arrays(dt1, dt2, k=1, options={}):
    opts = dict(options)
    opts.pop("crossCheck", None)
    return bf_match_arrays(dt1, dt2, k=k, options=opts)


def ratio_match_arrays(dt1, dt2, tau, options={}):
    """Classic Ratio-Match (the reference's baseline, ``Classic Matching.ipynb`` cell 3):
    brute-force 2-NN then ``m[0].distance / m[1].distance < tau`` in float64, on the device.
    Returns (query idx, train idx, distance, ratio) of the accepted matches, ascending query."""
    norm = _norm_type(options, dt1, dt2)
    _mask_option(options, dt1, dt2, "ratio_match_arrays", "the ratio test")
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _bank_pair(ctx, dt1, dt2, norm)
    try:
        return ctx.knn2_ratio(qb, tb, tau)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def mutual_ratio_match_arrays(dt1, dt2, tau, symmetric=False, options={}):
    """Mutual nearest neighbours that also pass the ratio test (hloc's "NN-ratio + mutual", kornia's ``match_smnn``, cv2's
    ``knnMatch(k=2)`` + ratio + crossCheck loop) in one call, ``fm_mutual_ratio``: query row i is kept iff
    ``d0 / d1 < tau`` on its 2-NN list and i is the nearest query row of its first neighbour (lowest index on ties);
    ``symmetric`` also asks the ratio test of that train row's own 2-NN list over the query rows.  ``options["normType"]``:
    NORM_L2 or NORM_HAMMING.  Returns (query idx, train idx, distance, ratio) ascending in query index; ``ratio`` is the
    larger of the two ratios in symmetric mode."""
    norm = _norm_type(options, dt1, dt2)
    _mask_option(options, dt1, dt2, "mutual_ratio_match_arrays", "the mutual ratio test")
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _bank_pair(ctx, dt1, dt2, norm)
    try:
        return ctx.mutual_ratio(qb, tb, tau, symmetric)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def bf_radius_match_arrays(dt1, dt2, maxDistance, options={}):
    """Array form of :func:`bf_radius_match`: ``(offsets int64[nq + 1], idx int32[n], dist float32[n])``; query row i's
    list is ``idx[offsets[i]:offsets[i + 1]]`` / ``dist[...]``.  ``maxDistance`` is a scalar (float32, as the cv2 binding
    passes it) or an array of one radius per query row."""
    if _norm_type(options, dt1, dt2) == NORM_HAMMING:
        raise ValueError("bf_radius_match: radiusMatch with NORM_HAMMING is not built here (NORM_L2 only): hamming_radius_match is the call")
    _mask_option(options, dt1, dt2, "bf_radius_match", "radiusMatch")
    _refuse_wide("bf_radius_match", "radiusMatch", dt1, dt2)
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _as_bank_pair(ctx, dt1, dt2)
    try:
        return ctx.radius_match(qb, tb, maxDistance)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def bf_radius_match(dt1, dt2, maxDistance, options={}):
    """ cv2.BFMatcher(NORM_L2).radiusMatch(dt1, dt2, maxDistance): a list of DMatch lists, one per query row """
    off, idx, dist = bf_radius_match_arrays(dt1, dt2, maxDistance, options=options)
    return [[DMatch(qi, idx[j], dist[j]) for j in range(off[qi], off[qi + 1])] for qi in range(off.shape[0] - 1)]


def bf_radius_match_masked_arrays(dt1, dt2, maxDistance, mask, options={}):
    """``cv2.BFMatcher(normType).radiusMatch(dt1, dt2, maxDistance, mask)`` as arrays: ``(offsets int64[nq + 1], idx int32[n],
    dist float32[n])`` -- the lists of the unmasked call that serves the operands with every entry whose pair ``mask`` forbids
    removed, nothing else changed (``fm_radius_match_masked``, on the matrix cores for every kind).  The call is chosen by
    ``options["normType"]`` and the row width: NORM_HAMMING (uint8 rows of 1 .. 64 bytes, or binary banks) is
    :func:`hamming_radius_match_arrays`'s, float rows of 129 .. 256 values (or wide banks) :func:`wide_radius_match_arrays`'s,
    everything else :func:`bf_radius_match_arrays`'s.  ``mask``: a uint8 / bool ``[nq, nt]`` array, nonzero = the pair may be
    listed, or a resident ``_ffi.Mask`` (``Context.mask``).  ``ValueError`` before anything is uploaded: what the unmasked call
    refuses for the operands, ``mask`` None, a mask of another shape or dtype, a collection's Mask, a wrong number of radii."""
    who = "bf_radius_match_masked"
    options = options or {}
    norm = _norm_type(options, dt1, dt2)
    wide = norm != NORM_HAMMING and (_is_wide(dt1) or _is_wide(dt2))
    if norm == NORM_HAMMING:
        q, qw, _ = _binary_operand(dt1)
        t, tw, _ = _binary_operand(dt2)
        if qw != tw:
            raise ValueError("%s: %d bytes per query row, %d per train row" % (who, qw, tw))
    elif wide:
        q, qw = _wide_operand(dt1, who)
        t, tw = _wide_operand(dt2, who)
        if qw != tw:
            raise ValueError("%s: %d values per query row, %d per train row" % (who, qw, tw))
    else:
        q, t = dt1, dt2
        for d in (q, t):
            if not isinstance(d, _ffi.Bank) and np.asarray(d).ndim != 2:
                raise ValueError("descriptors must be a 2-D [n, dim] array")
    if mask is None:
        raise ValueError("%s: mask is None (bf_radius_match, hamming_radius_match and wide_radius_match are the calls without one)" % who)
    mask = _mask_option({"mask": mask}, q, t, who)
    nq = _rows_of(q)
    if np.ndim(maxDistance) != 0 and np.asarray(maxDistance).reshape(-1).shape[0] != nq:
        raise ValueError("%s: %d radii for %d query rows" % (who, np.asarray(maxDistance).reshape(-1).shape[0], nq))
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _bank_pair(ctx, q, t, norm)
    try:
        if isinstance(mask, _ffi.Mask):
            return ctx.radius_match_masked(qb, tb, mask, maxDistance)
        with ctx.mask(qb.n, tb.n) as mk:
            return ctx.radius_match_masked(qb, tb, mk.set(mask), maxDistance)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def bf_radius_match_masked(dt1, dt2, maxDistance, mask, options={}):
    """ cv2.BFMatcher(normType).radiusMatch(dt1, dt2, maxDistance, mask): a list of DMatch lists, one per query row (an empty
    list where the mask permits nothing within maxDistance) """
    off, idx, dist = bf_radius_match_masked_arrays(dt1, dt2, maxDistance, mask, options=options)
    return [[DMatch(qi, idx[j], dist[j]) for j in range(off[qi], off[qi + 1])] for qi in range(off.shape[0] - 1)]


def _binary_operand(d):
    """A resident binary bank, or a uint8 [n, 1 .. 64] array -- ValueError before anything is uploaded.  Returns (operand, bytes, rows)."""
    if isinstance(d, _ffi.Bank):
        if d.kind != _ffi.FM_BANK_BIN:
            raise ValueError("hamming_radius_match takes binary banks (Context.bank_binary); bf_radius_match is the NORM_L2 call")
        return d, d.dim, d.n
    a = np.asarray(d)
    if a.ndim != 2:
        raise ValueError("descriptors must be a 2-D [n, bytes] array")
    if a.dtype != np.uint8:
        raise ValueError("hamming_radius_match needs uint8 descriptors (cv2 asserts CV_8U for NORM_HAMMING), got %s" % a.dtype)
    if not 1 <= a.shape[1] <= 64:
        raise ValueError("hamming_radius_match: binary descriptors have 1 .. 64 bytes per row, got %d" % a.shape[1])
    return a, a.shape[1], a.shape[0]


def hamming_radius_match_arrays(dt1, dt2, maxDistance, options={}):
    """``cv2.BFMatcher(cv2.NORM_HAMMING).radiusMatch(dt1, dt2, maxDistance)`` as arrays: ``(offsets int64[nq + 1], idx
    int32[n], dist float32[n])``; query row i's list is ``idx[offsets[i]:offsets[i + 1]]`` / ``dist[...]``, every train row
    with ``popcount(q XOR t) < maxDistance`` (a strict float32 compare; distances are integers, so ``h <= H`` is
    ``maxDistance = H + 0.5``), ascending by (h, train index).  ``dt1`` / ``dt2``: uint8 arrays of 1 .. 64 bytes per row or
    resident binary banks; ``maxDistance``: a scalar or one radius per query row.  ``ValueError`` before anything is
    uploaded: another dtype, widths that differ or lie outside 1 .. 64, a ``mask`` option, a wrong number of radii."""
    q, qw, nq = _binary_operand(dt1)
    t, tw, _ = _binary_operand(dt2)
    if qw != tw:
        raise ValueError("hamming_radius_match: %d bytes per query row, %d per train row" % (qw, tw))
    if options and options.get("mask") is not None:
        raise ValueError("hamming_radius_match: a mask is not built for radiusMatch (knnMatch takes one: bf_match)")
    if np.ndim(maxDistance) != 0 and np.asarray(maxDistance).reshape(-1).shape[0] != nq:
        raise ValueError("hamming_radius_match: %d radii for %d query rows" % (np.asarray(maxDistance).reshape(-1).shape[0], nq))
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _bank_pair(ctx, q, t, NORM_HAMMING)
    try:
        return ctx.hamming_radius_match(qb, tb, maxDistance)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def hamming_radius_match(dt1, dt2, maxDistance, options={}):
    """ cv2.BFMatcher(NORM_HAMMING).radiusMatch(dt1, dt2, maxDistance): a list of DMatch lists, one per query row """
    off, idx, dist = hamming_radius_match_arrays(dt1, dt2, maxDistance, options=options)
    return [[DMatch(qi, idx[j], dist[j]) for j in range(off[qi], off[qi + 1])] for qi in range(off.shape[0] - 1)]


# ---- NORM_HAMMING2: binary descriptors of 2-bit cells (ORB with WTA_K = 3 or 4) -----------------------------------------------
def _binary2_operand(d, who):
    """A resident NORM_HAMMING2 bank, or a uint8 [n, 1 .. 64] array -- ValueError before anything is uploaded.
    Returns (operand, bytes, rows)."""
    if isinstance(d, _ffi.Bank):
        if d.kind != _ffi.FM_BANK_BIN2:
            raise ValueError("%s takes NORM_HAMMING2 banks (Context.bank_binary2); a NORM_HAMMING bank (Context.bank_binary) "
                             "counts bits, not 2-bit cells, and goes to bf_match / hamming_radius_match" % who)
        return d, d.dim, d.n
    a = np.asarray(d)
    if a.ndim != 2:
        raise ValueError("%s: descriptors must be a 2-D [n, bytes] array" % who)
    if a.dtype != np.uint8:
        raise ValueError("%s needs uint8 descriptors (cv2 asserts CV_8U for NORM_HAMMING2), got %s" % (who, a.dtype))
    if not 1 <= a.shape[1] <= 64:
        raise ValueError("%s: binary descriptors have 1 .. 64 bytes per row, got %d" % (who, a.shape[1]))
    return a, a.shape[1], a.shape[0]


def _binary2_pair(dt1, dt2, who, options):
    """Both operands checked -- uint8, 2-D, 1 .. 64 columns, equal widths, no mask -- BEFORE the library is touched."""
    q, qw, nq = _binary2_operand(dt1, who)
    t, tw, _ = _binary2_operand(dt2, who)
    if qw != tw:
        raise ValueError("%s: %d bytes per query row, %d per train row" % (who, qw, tw))
    if options and options.get("mask") is not None:
        raise ValueError("%s: a mask is not built for NORM_HAMMING2" % who)
    return q, t, nq


class _Binary2Banks(object):
    """The two operands as NORM_HAMMING2 banks for one call (arrays are uploaded and closed again)."""
    def __init__(self, ctx, q, t):
        self.own = []
        try:
            self.banks = [self._one(ctx, d) for d in (q, t)]
        except Exception:
            self.close()
            raise

    def _one(self, ctx, d):
        if isinstance(d, _ffi.Bank):
            return d
        b = ctx.bank_binary2(d)
        self.own.append(b)
        return b

    def close(self):
        for b in self.own:
            b.close()
        self.own = []

    def __enter__(self):
        return self.banks

    def __exit__(self, *exc):
        self.close()


def hamming2_match_arrays(dt1, dt2, k=1, options={}):
    """``cv2.BFMatcher(cv2.NORM_HAMMING2, crossCheck).knnMatch(dt1, dt2, k)`` as arrays, :func:`bf_match_arrays`' shapes: the
    distance is the number of 2-bit cells (bits 2c, 2c + 1 of a byte) in which two rows differ, lists ascend by (distance,
    train index).  crossCheck is honoured at ``k == 1``.  ``dt1`` / ``dt2``: uint8 arrays of 1 .. 64 bytes per row or resident
    NORM_HAMMING2 banks (``Context.bank_binary2``); 1 <= k <= 8."""
    k = int(k)
    if k < 1:
        raise ValueError("hamming2_match: k must be at least 1")
    if k > 8:
        raise ValueError("hamming2_match: k = %d: the HIP path builds k-NN lists up to k = 8" % k)
    crossCheck = k == 1 and bool(options) and options.get("crossCheck", False) == True   # noqa: E712  (bf_match's rule)
    q, t, _ = _binary2_pair(dt1, dt2, "hamming2_match", options)
    ctx = _context(options)
    with _Binary2Banks(ctx, q, t) as (qb, tb):
        if crossCheck:
            return ctx.xcheck1(qb, tb)
        if k > 2:
            return ctx.knn(qb, tb, k)
        idx, dist = ctx.knn2(qb, tb)
        return idx[:, :k], dist[:, :k]


def hamming2_match(dt1, dt2, k=1, options={}):
    """ cv2.BFMatcher(NORM_HAMMING2[, crossCheck]).knnMatch(dt1, dt2, k): a list of DMatch lists, one per query row """
    idx, dist = hamming2_match_arrays(dt1, dt2, k=k, options=options)
    return matches_from_arrays(idx, dist)


def hamming2_ratio_match_arrays(dt1, dt2, tau, options={}):
    """:func:`ratio_match_arrays` under NORM_HAMMING2 (``fm_knn2_ratio`` on two NORM_HAMMING2 banks)."""
    q, t, _ = _binary2_pair(dt1, dt2, "hamming2_ratio_match_arrays", options)
    ctx = _context(options)
    with _Binary2Banks(ctx, q, t) as (qb, tb):
        return ctx.knn2_ratio(qb, tb, tau)


def hamming2_mutual_ratio_match_arrays(dt1, dt2, tau, symmetric=False, options={}):
    """:func:`mutual_ratio_match_arrays` under NORM_HAMMING2 (``fm_mutual_ratio`` on two NORM_HAMMING2 banks)."""
    q, t, _ = _binary2_pair(dt1, dt2, "hamming2_mutual_ratio_match_arrays", options)
    ctx = _context(options)
    with _Binary2Banks(ctx, q, t) as (qb, tb):
        return ctx.mutual_ratio(qb, tb, tau, symmetric)


def hamming2_radius_match_arrays(dt1, dt2, maxDistance, options={}):
    """``cv2.BFMatcher(cv2.NORM_HAMMING2).radiusMatch`` as arrays, :func:`hamming_radius_match_arrays`' shapes: every train row
    whose cell count is < ``maxDistance`` (strict, float32; a radius above 4 * bytes admits every row), ascending by
    (distance, train index).  ``maxDistance``: a scalar or one radius per query row."""
    q, t, nq = _binary2_pair(dt1, dt2, "hamming2_radius_match", options)
    if np.ndim(maxDistance) != 0 and np.asarray(maxDistance).reshape(-1).shape[0] != nq:
        raise ValueError("hamming2_radius_match: %d radii for %d query rows" % (np.asarray(maxDistance).reshape(-1).shape[0], nq))
    ctx = _context(options)
    with _Binary2Banks(ctx, q, t) as (qb, tb):
        return ctx.hamming_radius_match(qb, tb, maxDistance)


def hamming2_radius_match(dt1, dt2, maxDistance, options={}):
    """ cv2.BFMatcher(NORM_HAMMING2).radiusMatch(dt1, dt2, maxDistance): a list of DMatch lists, one per query row """
    off, idx, dist = hamming2_radius_match_arrays(dt1, dt2, maxDistance, options=options)
    return [[DMatch(qi, idx[j], dist[j]) for j in range(off[qi], off[qi + 1])] for qi in range(off.shape[0] - 1)]


class Hamming2Matcher(object):
    """What :func:`BFMatcher_create` returns for NORM_HAMMING2: ``match`` / ``knnMatch`` / ``radiusMatch`` with a train
    argument.  A train collection (``add`` / ``train`` / a call without a train argument) and masks are not built for this
    norm: ``ValueError``, before anything is uploaded."""

    def __init__(self, crossCheck=False, options={}):
        self.normType = NORM_HAMMING2
        self.crossCheck = bool(crossCheck)
        self.options = dict(options)

    def add(self, descriptors):
        raise ValueError("BFMatcher(NORM_HAMMING2).add: a train collection is not built for NORM_HAMMING2; pass a train argument")

    def train(self):
        raise ValueError("BFMatcher(NORM_HAMMING2).train: a train collection is not built for NORM_HAMMING2; pass a train argument")

    def _checked(self, who, trainDescriptors, mask, masks):
        if mask is not None or masks is not None:
            raise ValueError("BFMatcher(NORM_HAMMING2).%s: masks are not built for NORM_HAMMING2" % who)
        if trainDescriptors is None:
            raise ValueError("BFMatcher(NORM_HAMMING2).%s: a train collection is not built for NORM_HAMMING2; pass a train argument" % who)

    def knnMatch(self, queryDescriptors, trainDescriptors=None, k=None, mask=None, masks=None):
        if k is None and trainDescriptors is not None and np.isscalar(trainDescriptors):
            trainDescriptors, k = None, trainDescriptors          # knnMatch(query, k)
        self._checked("knnMatch", trainDescriptors, mask, masks)
        if k is None:
            raise TypeError("knnMatch: k is required")
        return hamming2_match(queryDescriptors, trainDescriptors, k=k, options=dict(self.options, crossCheck=self.crossCheck))

    def match(self, queryDescriptors, trainDescriptors=None, mask=None, masks=None):
        self._checked("match", trainDescriptors, mask, masks)
        return [m[0] for m in self.knnMatch(queryDescriptors, trainDescriptors, k=1) if m]

    def radiusMatch(self, queryDescriptors, trainDescriptors=None, maxDistance=None, mask=None, compactResult=False):
        if maxDistance is None and trainDescriptors is not None and np.isscalar(trainDescriptors):
            trainDescriptors, maxDistance = None, trainDescriptors
        self._checked("radiusMatch", trainDescriptors, mask, None)
        if maxDistance is None:
            raise TypeError("radiusMatch: maxDistance is required")
        return hamming2_radius_match(queryDescriptors, trainDescriptors, maxDistance, options=self.options)


def BFMatcher_create(normType=NORM_L2, crossCheck=False, options={}):
    """cv2's factory: :class:`BFMatcher` for NORM_L2 (4) and NORM_HAMMING (6), a :class:`Hamming2Matcher` for NORM_HAMMING2 (7)."""
    if normType == NORM_HAMMING2:
        return Hamming2Matcher(crossCheck=crossCheck, options=options)
    return BFMatcher(normType, crossCheck=crossCheck, options=options)


def hamming_fast_match_arrays(dt1, dt2, tau, options={}):
    """Fast-Match's accepted-match test on binary descriptors: ``(qidx int32[m], tidx int32[m], dist float32[m], ratio
    float64[m])``, ascending query index -- the pairs for which t is the cross-checked nearest neighbour of q under
    ``popcount(q XOR t)`` and ``dist / selfdist(q) < tau``, selfdist(q) the Hamming distance from q to its nearest OTHER row
    of ``dt1`` (computed on the device unless ``dt1`` is a resident bank that carries its own).  A query row with a duplicate
    in ``dt1`` (selfdist 0) is never accepted.  ``dt1`` / ``dt2``: uint8 arrays of 1 .. 64 bytes per row or resident binary
    banks.  ``ValueError`` before anything is uploaded: another dtype, widths that differ or lie outside 1 .. 64."""
    try:
        q, qw, _ = _binary_operand(dt1)
        t, tw, _ = _binary_operand(dt2)
    except ValueError as e:
        raise ValueError(str(e).replace("hamming_radius_match", "hamming_fast_match").replace("bf_radius_match", "fastmatch"))
    if qw != tw:
        raise ValueError("hamming_fast_match: %d bytes per query row, %d per train row" % (qw, tw))
    ctx = _context(options)
    qb, q_tmp, tb, t_tmp = _bank_pair(ctx, q, t, NORM_HAMMING)
    try:
        if q_tmp or not qb.has_selfdist:
            ctx.hamming_self_dist_batch([qb], want_host=False)
        return ctx.hamming_match_accepted(qb, tb, tau)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def hamming_fast_match(dt1, dt2, tau, options={}):
    """ The accepted matches of hamming_fast_match_arrays as a list of DMatch, ascending query index """
    qidx, tidx, dist, _ = hamming_fast_match_arrays(dt1, dt2, tau, options=options)
    return [DMatch(int(qidx[j]), int(tidx[j]), dist[j]) for j in range(qidx.shape[0])]


def _wide_operand(d, who):
    """A resident wide float bank, or a float32 / float64 [n, 129 .. 256] array -- ValueError before anything is uploaded.
    Returns (operand as it goes to the device, dim)."""
    if isinstance(d, _ffi.Bank):
        if d.kind != _ffi.FM_BANK_F32W:
            raise ValueError("%s takes wide float banks (FM_BANK_F32W, 129 .. 256 values per row); fastmatch / "
                             "hamming_fast_match serve the other kinds" % who)
        return d, d.dim
    a = np.asarray(d)
    if a.ndim != 2:
        raise ValueError("descriptors must be a 2-D [n, dim] array")
    if a.dtype not in (np.float32, np.float64):
        raise ValueError("%s needs float32 / float64 descriptors, got %s" % (who, a.dtype))
    if not 129 <= a.shape[1] <= 256:
        raise ValueError("%s: wide float descriptors have 129 .. 256 values per row, got %d" % (who, a.shape[1]))
    return np.ascontiguousarray(a, dtype=np.float32), a.shape[1]


def wide_fast_match_arrays(dt1, dt2, tau, options={}):
    """Fast-Match's accepted-match test on wide float descriptors (129 .. 256 values per row, SuperPoint and its kin):
    ``(qidx int32[m], tidx int32[m], dist float32[m], ratio float64[m])``, ascending query index -- the pairs for which t is
    the cross-checked nearest neighbour of q under the L2 distance and ``dist / selfdist(q) < tau``, selfdist(q) the distance
    from q to its nearest OTHER row of ``dt1`` (computed on the device unless ``dt1`` is a resident bank that carries its
    own).  A query row with an exact duplicate in ``dt1`` (selfdist 0) is never accepted.  ``dt1`` / ``dt2``: float32 / float64
    arrays or resident wide banks.  ``ValueError`` before anything is uploaded: another dtype, dims that differ or lie
    outside 129 .. 256."""
    q, qw = _wide_operand(dt1, "wide_fast_match")
    t, tw = _wide_operand(dt2, "wide_fast_match")
    if qw != tw:
        raise ValueError("wide_fast_match: %d values per query row, %d per train row" % (qw, tw))
    ctx = _context(options)
    qb, q_tmp = (q, False) if isinstance(q, _ffi.Bank) else (ctx.bank(q), True)
    try:
        tb, t_tmp = (t, False) if isinstance(t, _ffi.Bank) else (ctx.bank(t), True)
    except Exception:
        if q_tmp:
            qb.close()
        raise
    try:
        if q_tmp or not qb.has_selfdist:
            ctx.wide_self_dist_batch([qb], want_host=False)
        return ctx.wide_match_accepted(qb, tb, tau)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def wide_fast_match(dt1, dt2, tau, options={}):
    """ The accepted matches of wide_fast_match_arrays as a list of DMatch, ascending query index """
    qidx, tidx, dist, _ = wide_fast_match_arrays(dt1, dt2, tau, options=options)
    return [DMatch(int(qidx[j]), int(tidx[j]), dist[j]) for j in range(qidx.shape[0])]


def wide_radius_match_arrays(dt1, dt2, maxDistance, options={}):
    """``cv2.BFMatcher(cv2.NORM_L2).radiusMatch(dt1, dt2, maxDistance)`` on wide float descriptors (129 .. 256 values per row,
    SuperPoint and its kin) as arrays: ``(offsets int64[nq + 1], idx int32[n], dist float32[n])``; query row i's list is
    ``idx[offsets[i]:offsets[i + 1]]`` / ``dist[...]``, every train row with ``dist < maxDistance`` (a strict float32
    compare), ascending by (distance, train index).  ``dt1`` / ``dt2``: float32 / float64 arrays or resident wide banks;
    ``maxDistance``: a scalar or one radius per query row.  ``ValueError`` before anything is uploaded: another dtype (uint8
    rows included), dims that differ or lie outside 129 .. 256, a ``mask`` option, a wrong number of radii.
    (``bf_radius_match`` keeps refusing wide descriptors.)"""
    q, qw = _wide_operand(dt1, "wide_radius_match")
    t, tw = _wide_operand(dt2, "wide_radius_match")
    if qw != tw:
        raise ValueError("wide_radius_match: %d values per query row, %d per train row" % (qw, tw))
    if options and options.get("mask") is not None:
        raise ValueError("wide_radius_match: a mask is not built for radiusMatch")
    nq = _rows_of(q)
    if np.ndim(maxDistance) != 0 and np.asarray(maxDistance).reshape(-1).shape[0] != nq:
        raise ValueError("wide_radius_match: %d radii for %d query rows" % (np.asarray(maxDistance).reshape(-1).shape[0], nq))
    ctx = _context(options)
    qb, q_tmp = (q, False) if isinstance(q, _ffi.Bank) else (ctx.bank(q), True)
    try:
        tb, t_tmp = (t, False) if isinstance(t, _ffi.Bank) else (ctx.bank(t), True)
    except Exception:
        if q_tmp:
            qb.close()
        raise
    try:
        return ctx.wide_radius_match(qb, tb, maxDistance)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def wide_radius_match(dt1, dt2, maxDistance, options={}):
    """ radiusMatch on wide float descriptors (wide_radius_match_arrays): a list of DMatch lists, one per query row """
    off, idx, dist = wide_radius_match_arrays(dt1, dt2, maxDistance, options=options)
    return [[DMatch(qi, idx[j], dist[j]) for j in range(off[qi], off[qi + 1])] for qi in range(off.shape[0] - 1)]


def wide_bf_match_masked_arrays(dt1, dt2, mask, k=2, options=None):
    """``cv2.BFMatcher(cv2.NORM_L2).knnMatch(dt1, dt2, k, mask)`` on wide float descriptors (129 .. 256 values per row) as
    arrays: ``(idx int32[nq, k], dist float32[nq, k])``, row i the list ``bf_match_arrays(dt1, dt2, k)`` gives computed over
    the train rows ``mask`` permits for row i only -- the same distance bits, ascending (distance, train index), -1 / inf
    where fewer than k rows are permitted (``fm_wide_knn_masked``, on the matrix cores).  ``dt1`` / ``dt2``: float32 / float64
    arrays or resident wide banks; ``mask``: a uint8 / bool ``[nq, nt]`` array, nonzero = the pair may be matched, or a resident
    ``_ffi.Mask`` (``Context.mask``); k = 1 or 2.  ``ValueError`` before anything is uploaded: another dtype, dims that differ
    or lie outside 129 .. 256, a mask of another shape or dtype, another k.  (``bf_match`` keeps refusing a mask on wide
    descriptors.)"""
    who = "wide_bf_match_masked"
    q, qw = _wide_operand(dt1, who)
    t, tw = _wide_operand(dt2, who)
    if qw != tw:
        raise ValueError("%s: %d values per query row, %d per train row" % (who, qw, tw))
    k = int(k)
    if k < 1 or k > 2:
        raise ValueError("%s: k = %d: wide float descriptors take k = 1 or 2" % (who, k))
    if mask is None:
        raise ValueError("%s: mask is None (bf_match serves wide descriptors without a mask)" % who)
    mask = _mask_option({"mask": mask}, q, t, who)
    ctx = _context(options or {})
    qb, q_tmp = (q, False) if isinstance(q, _ffi.Bank) else (ctx.bank(q), True)
    try:
        tb, t_tmp = (t, False) if isinstance(t, _ffi.Bank) else (ctx.bank(t), True)
    except Exception:
        if q_tmp:
            qb.close()
        raise
    try:
        if isinstance(mask, _ffi.Mask):
            return ctx.wide_knn_masked(qb, tb, mask, k)
        with ctx.mask(qb.n, tb.n) as mk:
            return ctx.wide_knn_masked(qb, tb, mk.set(mask), k)
    finally:
        if q_tmp:
            qb.close()
        if t_tmp:
            tb.close()


def wide_bf_match_masked(dt1, dt2, mask, k=2, options=None):
    """ knnMatch under a mask on wide float descriptors (wide_bf_match_masked_arrays): bf_match's list of DMatch lists, one per
    query row, shorter where fewer than k train rows are permitted """
    idx, dist = wide_bf_match_masked_arrays(dt1, dt2, mask, k=k, options=options)
    return matches_from_arrays(idx, dist)


class BFMatcher(object):
    """``cv2.BFMatcher(normType, crossCheck)`` with cv2's method names.  With a train argument ``match`` / ``knnMatch`` /
    ``radiusMatch`` are :func:`bf_match` / :func:`bf_radius_match`; without one they run against the TRAIN COLLECTION
    built with ``add([d1, d2, ...])`` (``train()`` uploads it; implicit in the first match; ``clear()`` empties it) and
    every ``DMatch.imgIdx`` names the image of the hit (``fm_collection_*``: one sweep over all images, the earlier
    image wins a tie).  NORM_L2 collections hold uint8 or float32 images (float32 images whose values are all integers in
    0 .. 255 take the exact integer route until the first other image arrives; a float32 QUERY that is not integer valued
    against such a collection is refused by the library: upload the query's kind of images), NORM_HAMMING collections binary
    rows.  ``ValueError`` before anything is uploaded: a normType other than 4 / 6, ``match`` / ``knnMatch`` with crossCheck on a collection of more than one image
    (OpenCV asserts there too, as far as SURVEY.md Appendix A recalls), ``radiusMatch`` on a collection.
    ``matchEach`` is ``match`` against every image separately -- with crossCheck the mutual nearest neighbours image by image,
    the collection form crossCheck does have.
    ``knnMatch_arrays`` / ``knnMatchEach_arrays`` / ``matchEach_arrays`` / ``votes`` return NumPy arrays.  ``fastMatchEach`` / ``fastMatchEach_arrays``
    run Fast-Match's self-distance test against every image of the collection (NORM_L2 only).  ``matchPairs`` /
    ``matchPairs_arrays`` match the added images against each other (the match graph), one call for any number of pairs."""

    def __init__(self, normType=NORM_L2, crossCheck=False, options={}):
        if normType not in (NORM_L2, NORM_HAMMING):
            raise ValueError("normType %r: BFMatcher builds NORM_L2 (4) and NORM_HAMMING (6) only%s"
                             % (normType, " (NORM_HAMMING2: BFMatcher_create(7) returns the matcher that serves it)" if normType == 7 else ""))
        self.normType = normType
        self.crossCheck = bool(crossCheck)
        self.options = dict(options)
        self.options["normType"] = normType
        self._images = []
        self._coll = None          # (_ffi.Collection, number of images it holds)
        self._uploaded = 0
        self._wide = False         # the images came through add_wide: matchPairs and the *WideEach calls are what it serves

    # -- bookkeeping (host only) ---------------------------------------------------------
    def add(self, descriptors):
        if self._wide:
            raise ValueError("BFMatcher.add: the collection holds wide float images (add_wide); wide and other images do not mix")
        imgs = []
        for d in descriptors:
            a = np.asarray(d)
            if a.ndim != 2:
                raise ValueError("BFMatcher.add: every image's descriptors must be a 2-D [n, dim] array")
            if self.normType == NORM_HAMMING and a.dtype != np.uint8:
                raise ValueError("NORM_HAMMING needs uint8 descriptors (cv2 asserts CV_8U), got %s" % a.dtype)
            _refuse_wide("BFMatcher.add", "a train collection (wide float images go in through add_wide)", a)
            for b in self._images + imgs:
                if a.shape[0] and b.shape[0] and (b.shape[1] != a.shape[1] or (b.dtype == np.uint8) != (a.dtype == np.uint8)):
                    raise ValueError("BFMatcher.add: images of one collection share a width and a dtype (cv2 raises at match time)")
            imgs.append(a)
        self._images.extend(imgs)

    def add_wide(self, descriptors):
        """``add`` for WIDE float images: every entry a [n, dim] float array with 129 <= dim <= 256 (learned 256-D descriptors;
        n may be 0), one width per collection, NORM_L2.  A collection takes either ``add`` or ``add_wide`` images; a wide one
        (``fm_collection_add_wide``) serves ``matchPairs`` / ``matchPairs_arrays`` and, for a wide query,
        ``mutualRatioMatchWideEach`` / ``mutualRatioMatchWideEach_arrays`` / ``knnMatchWideEach_arrays`` and, against all images at
        once, ``knnMatchWide`` / ``knnMatchWide_arrays`` / ``ratioMatchWide_arrays`` / ``votesWide``; every other collection
        method raises ``ValueError`` before anything is uploaded."""
        if self.normType != NORM_L2:
            raise ValueError("BFMatcher.add_wide: wide float images are NORM_L2 descriptors")
        if self._images and not self._wide:
            raise ValueError("BFMatcher.add_wide: the collection holds images of another kind; wide and other images do not mix")
        imgs = []
        for d in descriptors:
            a = np.asarray(d)
            if a.ndim != 2:
                raise ValueError("BFMatcher.add_wide: every image's descriptors must be a 2-D [n, dim] array")
            if a.dtype == np.uint8 or not 129 <= a.shape[1] <= 256:
                raise ValueError("BFMatcher.add_wide: wide images are float arrays of 129 .. 256 values per row, got %s [%d, %d]"
                                 % (a.dtype, a.shape[0], a.shape[1]))
            for b in self._images + imgs:
                if b.shape[1] != a.shape[1]:
                    raise ValueError("BFMatcher.add_wide: the images of one collection share a width")
            imgs.append(np.ascontiguousarray(a, dtype=np.float32))
        self._images.extend(imgs)
        if imgs:
            self._wide = True

    def clear(self):
        self._images = []
        self._uploaded = 0
        self._wide = False
        if self._coll is not None:
            self._coll.clear()

    def empty(self):
        return len(self._images) == 0

    def getTrainDescriptors(self):
        return list(self._images)

    # -- the collection on the device ------------------------------------------------------
    def _check_collection(self, who):
        if self.empty():
            raise ValueError("%s: no train descriptors (add() some, or pass a train array)" % who)
        if self._wide and who not in ("BFMatcher.train", "BFMatcher.matchPairs", "BFMatcher.mutualRatioMatchWideEach",
                                      "BFMatcher.knnMatchWideEach", "BFMatcher.wideFastMatchEach", "BFMatcher.knnMatchWide",
                                      "BFMatcher.ratioMatchWide", "BFMatcher.votesWide"):
            raise ValueError("%s is not built for a wide collection (images of 129 .. 256 values per row, add_wide): "
                             "matchPairs, matchPairs_arrays and, for a wide query, mutualRatioMatchWideEach(_arrays), "
                             "wideFastMatchEach(_arrays), knnMatchWideEach_arrays and, against all images at once, "
                             "knnMatchWide(_arrays), ratioMatchWide_arrays and votesWide are" % who)

    def train(self):
        self._check_collection("BFMatcher.train")
        ctx = _context(self.options)
        if self._coll is None or self._coll.handle is None or self._coll.ctx is not ctx:
            self._coll = ctx.collection()
            self._uploaded = 0
        for a in self._images[self._uploaded:]:
            if self.normType == NORM_HAMMING:
                self._coll.add_binary(a)
            elif self._wide:
                self._coll.add_wide(a)
            else:
                self._coll.add(a)
            self._uploaded += 1
        self._coll.train()
        return self._coll

    def _query(self, ctx, q):
        if isinstance(q, _ffi.Bank):
            return q, False
        a = np.asarray(q)
        if a.ndim != 2:
            raise ValueError("descriptors must be a 2-D [n, dim] array")
        if self.normType == NORM_HAMMING:
            return ctx.bank_binary(a), True
        # (a float32-route collection takes a float32-route query, integer valued or not)
        return ctx.bank(a, float_route=self._coll.info()[3] == _ffi.FM_BANK_F32 and a.dtype != np.uint8), True

    def _check_masks(self, masks, queryDescriptors):
        """cv2's ``masks``: one uint8 / bool [nq, rows of the image] array per added image, None = everything -- checked before
        anything is uploaded.  (A resident ``_ffi.Mask`` of the collection passes as it is.)"""
        if self.crossCheck:
            raise ValueError("BFMatcher.knnMatch: masks with crossCheck are not built")
        if isinstance(masks, _ffi.Mask):
            return masks
        masks = list(masks)
        if len(masks) != len(self._images):
            raise ValueError("BFMatcher.knnMatch: masks has %d entries, the collection %d images" % (len(masks), len(self._images)))
        nq = _rows_of(queryDescriptors)
        return [None if m is None else _mask_array(m, nq, self._images[i].shape[0], "BFMatcher.knnMatch: masks[%d]" % i)
                for i, m in enumerate(masks)]

    def knnMatch_arrays(self, queryDescriptors, k, masks=None):
        """(img, idx, dist) [nq, k] against the collection: ``imgIdx``, ``trainIdx`` inside that image, distance; -1 / -1 / inf
        where the collection has fewer than k (permitted) rows.  ``masks``: see the module docstring."""
        k = int(k)
        if k < 1 or k > 8:
            raise ValueError("BFMatcher.knnMatch: k = %d: the HIP path builds k-NN lists for 1 <= k <= 8" % k)
        self._check_collection("BFMatcher.knnMatch")
        if self.crossCheck and len(self._images) > 1:
            raise ValueError("BFMatcher: crossCheck has no stacked collection form (more than one train image); matchEach runs it "
                             "image by image")
        if self.normType == NORM_HAMMING and np.asarray(queryDescriptors).dtype != np.uint8 and not isinstance(queryDescriptors, _ffi.Bank):
            raise ValueError("NORM_HAMMING needs uint8 descriptors (cv2 asserts CV_8U), got %s" % np.asarray(queryDescriptors).dtype)
        if masks is not None:
            masks = self._check_masks(masks, queryDescriptors)
        if self.crossCheck and k == 1:
            tidx, dist = bf_match_arrays(queryDescriptors, self._images[0], k=1, options=dict(self.options, crossCheck=True))
            return np.where(tidx >= 0, 0, -1).astype(np.int32)[:, None], tidx[:, None], dist[:, None]
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            if isinstance(masks, _ffi.Mask):
                return coll.knn_masked(qb, masks, k)
            if masks is not None:
                with coll.mask(qb.n) as mk:
                    for i, m in enumerate(masks):
                        if m is None:
                            mk.set_all(True, img=i)
                        else:
                            mk.set(m, img=i)
                    return coll.knn_masked(qb, mk, k)
            return coll.knn(qb, k)
        finally:
            if tmp:
                qb.close()

    def knnMatchEach_arrays(self, queryDescriptors):
        """(idx, dist) [n_images, nq, 2]: the 2-NN lists of the query inside every image separately."""
        self._check_collection("BFMatcher.knnMatchEach")
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            return coll.knn2_each(qb)
        finally:
            if tmp:
                qb.close()

    def votes(self, queryDescriptors, tau, mode=0):
        """int64[n_images]: query rows that pass the ratio test d0 / d1 < tau per image (mode 0: on the 2-NN lists over all
        images, counted at the first neighbour's image; 1: on every image's own 2-NN lists)."""
        self._check_collection("BFMatcher.votes")
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            return coll.votes(qb, tau, mode)
        finally:
            if tmp:
                qb.close()

    def fastMatchEach_arrays(self, queryDescriptors, tau):
        """A list of (qidx, tidx, dist, ratio) per image: Fast-Match's accepted matches of the query inside every image
        separately (``Collection.match_accepted_each``)."""
        if self.normType == NORM_HAMMING:
            raise ValueError("BFMatcher.fastMatchEach is the NORM_L2 call: hammingFastMatchEach runs the self-distance test of a "
                             "NORM_HAMMING matcher")
        self._check_collection("BFMatcher.fastMatchEach")
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            if tmp or not qb.has_selfdist:
                coll.ctx.self_dist_batch([qb], want_host=False)        # attached on the device, nothing comes back
            return coll.match_accepted_each(qb, tau)
        finally:
            if tmp:
                qb.close()

    def fastMatchEach(self, queryDescriptors, tau):
        """Fast-Match's accepted-match test against the collection, image by image: one list of ``DMatch`` per added image
        (``imgIdx`` set), holding the matches (q, t) for which t is the cross-checked nearest neighbour of q INSIDE that image
        and ``dist(q, t) / selfdist(q) < tau`` -- what ``fastmatch``'s first round accepts for the pair (query, image).  The
        query's self distances are computed on the device.  The test is cross-checked by definition: the matcher's
        ``crossCheck`` flag is ignored.  ``ValueError`` for a NORM_HAMMING matcher and for an empty collection, before
        anything is uploaded."""
        out = []
        for i, (qidx, tidx, dist, _) in enumerate(self.fastMatchEach_arrays(queryDescriptors, tau)):
            out.append([DMatch(int(qidx[j]), int(tidx[j]), dist[j], i) for j in range(qidx.shape[0])])
        return out

    def hammingFastMatchEach_arrays(self, queryDescriptors, tau):
        """``fastMatchEach_arrays`` of a NORM_HAMMING matcher: a list of (qidx, tidx, dist, ratio) per image, slot i equal to
        ``hamming_fast_match_arrays(query, image_i, tau)`` (``Collection.hamming_match_accepted_each``).  ``ValueError`` on a
        NORM_L2 matcher, another dtype and an empty collection, before anything is uploaded."""
        if self.normType != NORM_HAMMING:
            raise ValueError("BFMatcher.hammingFastMatchEach needs a NORM_HAMMING matcher: fastMatchEach is the NORM_L2 call")
        if not isinstance(queryDescriptors, _ffi.Bank) and np.asarray(queryDescriptors).dtype != np.uint8:
            raise ValueError("NORM_HAMMING needs uint8 descriptors (cv2 asserts CV_8U), got %s" % np.asarray(queryDescriptors).dtype)
        self._check_collection("BFMatcher.hammingFastMatchEach")
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            if tmp or not qb.has_selfdist:
                coll.ctx.hamming_self_dist_batch([qb], want_host=False)        # attached on the device, nothing comes back
            return coll.hamming_match_accepted_each(qb, tau)
        finally:
            if tmp:
                qb.close()

    def hammingFastMatchEach(self, queryDescriptors, tau):
        """Fast-Match's accepted-match test of a NORM_HAMMING matcher against its collection, image by image: one list of
        ``DMatch`` per added image (``imgIdx`` set) -- t is the cross-checked nearest neighbour of q inside that image and
        ``popcount(q XOR t) / selfdist(q) < tau``, selfdist(q) the Hamming distance from q to its nearest OTHER query row
        (computed on the device).  A query row with a duplicate (selfdist 0) is never accepted."""
        out = []
        for i, (qidx, tidx, dist, _) in enumerate(self.hammingFastMatchEach_arrays(queryDescriptors, tau)):
            out.append([DMatch(int(qidx[j]), int(tidx[j]), dist[j], i) for j in range(qidx.shape[0])])
        return out

    def matchEach_arrays(self, queryDescriptors):
        """(tidx int32, dist float32) [n_images, nq]: ``match`` of the query against every image of the collection separately
        (-1 / inf: no match in that image).  With ``crossCheck`` the mutual nearest neighbours inside every image
        (``Collection.xcheck1_each``), without it the nearest row of every image (first column of ``Collection.knn2_each``)."""
        self._check_collection("BFMatcher.matchEach")
        if self.normType == NORM_HAMMING and not isinstance(queryDescriptors, _ffi.Bank) and np.asarray(queryDescriptors).dtype != np.uint8:
            raise ValueError("NORM_HAMMING needs uint8 descriptors (cv2 asserts CV_8U), got %s" % np.asarray(queryDescriptors).dtype)
        if not isinstance(queryDescriptors, _ffi.Bank) and np.asarray(queryDescriptors).ndim != 2:
            raise ValueError("descriptors must be a 2-D [n, dim] array")
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            if self.crossCheck:
                return coll.xcheck1_each(qb)
            idx, dist = coll.knn2_each(qb)
            return np.ascontiguousarray(idx[:, :, 0]), np.ascontiguousarray(dist[:, :, 0])
        finally:
            if tmp:
                qb.close()

    def matchEach(self, queryDescriptors):
        """``[BFMatcher(normType, crossCheck).match(query, t) for t in images]`` as one call against the collection: one list
        of ``DMatch`` per added image, ``imgIdx`` set, ascending query index.  NORM_L2 and NORM_HAMMING; with ``crossCheck``
        one reverse sweep serves all images (``fm_collection_xcheck1_each``).  ``ValueError`` for an empty collection and
        for a query of the wrong dtype, before anything is uploaded."""
        tidx, dist = self.matchEach_arrays(queryDescriptors)
        return [[DMatch(int(qi), int(tidx[i, qi]), dist[i, qi], i) for qi in np.nonzero(tidx[i] >= 0)[0]]
                for i in range(tidx.shape[0])]

    def mutualRatioMatchEach_arrays(self, queryDescriptors, tau, symmetric=False):
        """A list of (qidx, tidx, dist, ratio) per image: the mutual nearest neighbours of the query inside every image
        separately that also pass the ratio test there (``Collection.mutual_ratio_each``; slot i equals
        ``mutual_ratio_match_arrays(query, image_i, tau, symmetric)``).  NORM_L2 and NORM_HAMMING."""
        self._check_collection("BFMatcher.mutualRatioMatchEach")
        if self.normType == NORM_HAMMING and not isinstance(queryDescriptors, _ffi.Bank) and np.asarray(queryDescriptors).dtype != np.uint8:
            raise ValueError("NORM_HAMMING needs uint8 descriptors (cv2 asserts CV_8U), got %s" % np.asarray(queryDescriptors).dtype)
        if not isinstance(queryDescriptors, _ffi.Bank) and np.asarray(queryDescriptors).ndim != 2:
            raise ValueError("descriptors must be a 2-D [n, dim] array")
        coll = self.train()
        qb, tmp = self._query(coll.ctx, queryDescriptors)
        try:
            return coll.mutual_ratio_each(qb, tau, symmetric)
        finally:
            if tmp:
                qb.close()

    def mutualRatioMatchEach(self, queryDescriptors, tau, symmetric=False):
        """``knnMatch(k=2)`` + ratio test + crossCheck against every image of the collection separately, as one call: one list
        of ``DMatch`` per added image, ``imgIdx`` set, ascending query index (``fm_collection_mutual_ratio_each``: one
        restricted reverse sweep serves all images).  The matcher's ``crossCheck`` flag is ignored: the test is mutual by
        definition.  ``ValueError`` for an empty collection and for a query of the wrong dtype, before anything is uploaded."""
        out = []
        for i, (qidx, tidx, dist, _) in enumerate(self.mutualRatioMatchEach_arrays(queryDescriptors, tau, symmetric)):
            out.append([DMatch(int(qidx[j]), int(tidx[j]), dist[j], i) for j in range(qidx.shape[0])])
        return out

    def _wide_query(self, who, queryDescriptors):
        """The checks of the wide-query calls, before anything is uploaded: NORM_L2, a wide collection, a float query of the
        collection's width (or a resident wide bank of it).  Returns the query as it goes to the device."""
        if self.normType != NORM_L2:
            raise ValueError("%s: wide float descriptors are NORM_L2 descriptors" % who)
        self._check_collection(who)
        if not self._wide:
            raise ValueError("%s: the collection is not a wide one (add_wide); mutualRatioMatchEach / knnMatchEach_arrays "
                             "serve the other kinds" % who)
        dim = self._images[0].shape[1]
        if isinstance(queryDescriptors, _ffi.Bank):
            if queryDescriptors.kind != _ffi.FM_BANK_F32W or queryDescriptors.dim != dim:
                raise ValueError("%s: the query bank is not a wide float bank of the collection's width %d" % (who, dim))
            return queryDescriptors
        a = np.asarray(queryDescriptors)
        if a.ndim != 2 or a.dtype.kind != "f" or a.shape[1] != dim:
            raise ValueError("%s: the query is a float array [nq, %d] (the collection's width), got %s %s"
                             % (who, dim, a.dtype, list(a.shape)))
        return np.ascontiguousarray(a, dtype=np.float32)

    def mutualRatioMatchWideEach_arrays(self, queryDescriptors, tau, symmetric=False):
        """A wide query ([nq, dim] floats, or a resident wide bank) against every image of a WIDE collection (``add_wide``):
        a list of (qidx, tidx, dist, ratio) per image, slot i equal to ``mutual_ratio_match_arrays(query, image_i, tau,
        symmetric)`` (``Collection.wide_mutual_ratio_each``: one call, whatever the number of images).  ``ValueError`` before
        anything is uploaded: a collection that is not wide, a query that is not a float array of the collection's width,
        a norm other than NORM_L2."""
        q = self._wide_query("BFMatcher.mutualRatioMatchWideEach", queryDescriptors)
        coll = self.train()
        qb, tmp = (q, False) if isinstance(q, _ffi.Bank) else (coll.ctx.bank(q), True)
        try:
            return coll.wide_mutual_ratio_each(qb, tau, symmetric)
        finally:
            if tmp:
                qb.close()

    def mutualRatioMatchWideEach(self, queryDescriptors, tau, symmetric=False):
        """One list of ``DMatch`` per added image of :meth:`mutualRatioMatchWideEach_arrays`: ``queryIdx`` the query row,
        ``trainIdx`` the row inside the image, ``imgIdx`` the image, ascending ``queryIdx``."""
        out = []
        for i, (qidx, tidx, dist, _) in enumerate(self.mutualRatioMatchWideEach_arrays(queryDescriptors, tau, symmetric)):
            out.append([DMatch(int(qidx[j]), int(tidx[j]), dist[j], i) for j in range(qidx.shape[0])])
        return out

    def wideFastMatchEach_arrays(self, queryDescriptors, tau):
        """``fastMatchEach_arrays`` of a WIDE collection (``add_wide``): a list of (qidx, tidx, dist, ratio) per image, slot i
        equal to ``wide_fast_match_arrays(query, image_i, tau)`` (``Collection.wide_match_accepted_each``).  The query's self
        distances are computed on the device unless it is a resident bank that carries them.  The refusals are
        :meth:`mutualRatioMatchWideEach_arrays`'."""
        q = self._wide_query("BFMatcher.wideFastMatchEach", queryDescriptors)
        coll = self.train()
        qb, tmp = (q, False) if isinstance(q, _ffi.Bank) else (coll.ctx.bank(q), True)
        try:
            if tmp or not qb.has_selfdist:
                coll.ctx.wide_self_dist_batch([qb], want_host=False)          # attached on the device, nothing comes back
            return coll.wide_match_accepted_each(qb, tau)
        finally:
            if tmp:
                qb.close()

    def wideFastMatchEach(self, queryDescriptors, tau):
        """Fast-Match's accepted-match test of a wide query against a WIDE collection, image by image: one list of ``DMatch``
        per added image (``imgIdx`` set) -- t is the cross-checked nearest neighbour of q inside that image and
        ``dist(q, t) / selfdist(q) < tau``.  A query row with an exact duplicate (selfdist 0) is never accepted."""
        out = []
        for i, (qidx, tidx, dist, _) in enumerate(self.wideFastMatchEach_arrays(queryDescriptors, tau)):
            out.append([DMatch(int(qidx[j]), int(tidx[j]), dist[j], i) for j in range(qidx.shape[0])])
        return out

    def knnMatchWideEach_arrays(self, queryDescriptors):
        """(idx int32, dist float32) [n_images, nq, 2]: the two nearest rows of every image of a WIDE collection for every row
        of a wide query, slot i equal to ``bf_match_arrays(query, image_i, k=2)`` (``Collection.wide_knn2_each``).  The
        refusals are :meth:`mutualRatioMatchWideEach_arrays`'."""
        q = self._wide_query("BFMatcher.knnMatchWideEach", queryDescriptors)
        coll = self.train()
        qb, tmp = (q, False) if isinstance(q, _ffi.Bank) else (coll.ctx.bank(q), True)
        try:
            return coll.wide_knn2_each(qb)
        finally:
            if tmp:
                qb.close()

    def _wide_stacked(self, who, queryDescriptors, call):
        """``call(collection, query bank)`` behind :meth:`_wide_query`'s checks: the wide calls against ALL images at once."""
        q = self._wide_query(who, queryDescriptors)
        coll = self.train()
        qb, tmp = (q, False) if isinstance(q, _ffi.Bank) else (coll.ctx.bank(q), True)
        try:
            return call(coll, qb)
        finally:
            if tmp:
                qb.close()

    def knnMatchWide_arrays(self, queryDescriptors, k):
        """(img, idx, dist) [nq, k], k = 1 or 2, of a wide query against ALL images of a WIDE collection (``add_wide``) at once:
        ``imgIdx``, ``trainIdx`` inside that image, distance -- ``bf_match_arrays(query, the images' rows concatenated, k)``
        with every hit located; -1 / -1 / inf where the collection has fewer than k rows (``Collection.wide_knn``).
        ``ValueError`` before anything is uploaded: k outside 1, 2, and :meth:`mutualRatioMatchWideEach_arrays`' refusals."""
        k = int(k)
        if k < 1 or k > 2:
            raise ValueError("BFMatcher.knnMatchWide: k = %d: wide float descriptors get k-NN lists for k = 1, 2" % k)
        return self._wide_stacked("BFMatcher.knnMatchWide", queryDescriptors, lambda coll, qb: coll.wide_knn(qb, k))

    def knnMatchWide(self, queryDescriptors, k):
        """``cv2.BFMatcher.knnMatch(query, k)`` against a WIDE collection: one list of up to k ``DMatch`` per query row, nearest
        first, ``imgIdx`` the image and ``trainIdx`` the row inside it (:meth:`knnMatchWide_arrays`)."""
        img, idx, dist = self.knnMatchWide_arrays(queryDescriptors, k)
        return [[DMatch(qi, idx[qi, j], dist[qi, j], img[qi, j]) for j in range(idx.shape[1]) if idx[qi, j] >= 0]
                for qi in range(idx.shape[0])]

    def ratioMatchWide_arrays(self, queryDescriptors, tau):
        """(qidx, img, tidx, dist, ratio) of the query rows whose 2-NN list over ALL images of a WIDE collection passes Lowe's
        test d0 / d1 < tau, ascending ``qidx`` (``Collection.wide_knn2_ratio``).  The refusals are
        :meth:`mutualRatioMatchWideEach_arrays`'."""
        return self._wide_stacked("BFMatcher.ratioMatchWide", queryDescriptors, lambda coll, qb: coll.wide_knn2_ratio(qb, tau))

    def votesWide(self, queryDescriptors, tau, mode=0):
        """:meth:`votes` of a wide query on a WIDE collection: int64[n_images] (``Collection.wide_votes``; mode 0: the test on
        the lists over all images, counted at the first neighbour's image; 1: on every image's own 2-NN lists).  The refusals
        are :meth:`mutualRatioMatchWideEach_arrays`', and a mode other than 0, 1."""
        if mode not in (0, 1):
            raise ValueError("BFMatcher.votesWide: mode must be 0 (stacked lists) or 1 (per-image lists)")
        return self._wide_stacked("BFMatcher.votesWide", queryDescriptors, lambda coll, qb: coll.wide_votes(qb, tau, mode))

    def matchPairs_arrays(self, pairs=None, ratio=0.8, symmetric=False):
        """The added images matched AGAINST EACH OTHER -- the match graph of structure from motion and stitching (COLMAP's
        exhaustive / sequential matchers, ``cv2.detail.BestOf2NearestMatcher``): ``(pairs int32 [n_pairs, 2], [(qidx, tidx,
        dist, ratio) per pair])``.  ``pairs``: ordered (a, b) image indices, None = every a < b in lexicographic order; entry
        p equals ``mutual_ratio_match_arrays(image_a, image_b, ratio, symmetric)``, ``qidx`` the row inside image a, ``tidx``
        inside image b (``Collection.pairs_mutual_ratio``: one call, whatever the number of pairs).  NORM_L2 and
        NORM_HAMMING.  ``ValueError`` before anything is uploaded: a matcher made with ``crossCheck=True`` (the call is mutual
        by itself), an empty collection, a malformed ``pairs`` (not [n_pairs, 2] integers, an index outside the images)."""
        if self.crossCheck:
            raise ValueError("BFMatcher.matchPairs: the call is mutual by itself; make the matcher with crossCheck=False")
        self._check_collection("BFMatcher.matchPairs")
        ni = len(self._images)
        if pairs is None:
            arr = np.array([(a, b) for a in range(ni) for b in range(a + 1, ni)], np.int32).reshape(-1, 2)
        else:
            arr = _ffi.pairs_array(pairs, ni)
        coll = self.train()
        return arr, coll.pairs_mutual_ratio(None if pairs is None else arr, ratio, symmetric)

    def matchPairs(self, pairs=None, ratio=0.8, symmetric=False):
        """``{(a, b): [DMatch]}`` of :meth:`matchPairs_arrays`: ``queryIdx`` is the row inside image a, ``trainIdx`` the row
        inside image b, ``imgIdx`` = b, ascending ``queryIdx``.  A pair listed more than once keeps one entry (its lists are
        equal)."""
        arr, res = self.matchPairs_arrays(pairs, ratio, symmetric)
        out = {}
        for (a, b), (qidx, tidx, dist, _) in zip(arr.tolist(), res):
            out[(a, b)] = [DMatch(int(qidx[j]), int(tidx[j]), dist[j], b) for j in range(qidx.shape[0])]
        return out

    # -- cv2's matching methods ------------------------------------------------------------
    def knnMatch(self, queryDescriptors, trainDescriptors=None, k=None, mask=None, masks=None):
        if k is None and trainDescriptors is not None and np.isscalar(trainDescriptors):
            trainDescriptors, k = None, trainDescriptors          # knnMatch(query, k)
        if k is None:
            raise TypeError("knnMatch: k is required")
        if trainDescriptors is not None:
            if masks is not None:
                raise ValueError("BFMatcher.knnMatch: masks goes with the train collection; a train argument takes mask")
            opts = dict(self.options, crossCheck=self.crossCheck)
            if mask is not None:
                opts["mask"] = mask
            return bf_match(queryDescriptors, trainDescriptors, k=k, options=opts)
        if mask is not None:
            raise ValueError("BFMatcher.knnMatch: mask goes with a train argument; the train collection takes masks (one per image)")
        if masks is None:
            img, idx, dist = self.knnMatch_arrays(queryDescriptors, k)
        else:
            img, idx, dist = self.knnMatch_arrays(queryDescriptors, k, masks=masks)
        return [[DMatch(qi, idx[qi, j], dist[qi, j], img[qi, j]) for j in range(idx.shape[1]) if idx[qi, j] >= 0]
                for qi in range(idx.shape[0])]

    def match(self, queryDescriptors, trainDescriptors=None, mask=None, masks=None):
        if mask is None and masks is None:
            return [m[0] for m in self.knnMatch(queryDescriptors, trainDescriptors, k=1) if m]
        return [m[0] for m in self.knnMatch(queryDescriptors, trainDescriptors, k=1, mask=mask, masks=masks) if m]

    def radiusMatch(self, queryDescriptors, trainDescriptors=None, maxDistance=None, mask=None, compactResult=False):
        """cv2's radiusMatch(query, train, maxDistance, mask, compactResult).  Without ``mask`` and ``compactResult`` the call is
        what it was before masks existed (:func:`bf_radius_match`).  ``mask``: :func:`bf_radius_match_masked`'s, on every kind of
        descriptor the matcher's normType takes.  ``compactResult`` = True drops the lists of the query rows whose mask row is
        entirely zero -- OpenCV's rule as recalled, not verified -- so the result may have fewer than nq lists (every DMatch keeps
        its queryIdx); without a mask it drops nothing."""
        if maxDistance is None and trainDescriptors is not None and np.isscalar(trainDescriptors):
            trainDescriptors, maxDistance = None, trainDescriptors
        if trainDescriptors is None:
            raise ValueError("BFMatcher.radiusMatch: radiusMatch on a collection returns arrays, not DMatch lists, for now: "
                             "Collection.radius_match (_ffi / torchmatch) is the array-form route; or pass a train array")
        if maxDistance is None:
            raise TypeError("radiusMatch: maxDistance is required")
        if mask is None:
            return bf_radius_match(queryDescriptors, trainDescriptors, maxDistance, options=self.options)
        if compactResult and isinstance(mask, _ffi.Mask):
            raise ValueError("BFMatcher.radiusMatch: compactResult needs the mask as an array (a resident Mask's rows are on the device)")
        out = bf_radius_match_masked(queryDescriptors, trainDescriptors, maxDistance, mask, options=self.options)
        if compactResult:
            keep = np.asarray(mask).astype(bool).any(axis=1)
            out = [m for qi, m in enumerate(out) if keep[qi]]
        return out


# ---- SIFT stays in OpenCV on the host -------------------------------------------------

def sift():
    try:
        import cv2
    except ImportError:
        raise Exception("Can't find SIFT: OpenCV (cv2) is not installed; pass pre-extracted "
                        "features (cache.Feature_Image / Metric_Cache.from_arrays) instead")
    if hasattr(cv2, "SIFT_create"):
        return cv2.SIFT_create()
    if hasattr(cv2, "SIFT"):
        return cv2.SIFT()
    if hasattr(cv2, "xfeatures2d"):
        return cv2.xfeatures2d.SIFT_create()
    raise Exception("Can't find SIFT")


def get_features(data, feature_type="SIFT"):
    return sift().detectAndCompute(data, None)


def get_keypoints(data, feature_type="SIFT"):
    return sift().detect(data)
