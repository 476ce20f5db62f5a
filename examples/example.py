"""The reference's README example (README.md:34-55 / Example.ipynb) on the MI355X path, with a
synthetic pre-extracted image pair standing in for SIFT (cv2 is not required):

    python examples/example.py            # needs an MI355X

With OpenCV installed, replace the two `from_arrays` / `Feature_Image` lines by
`cache.Metric_Cache(path_query)` and `imaging.open_img(path_target)` as in the reference.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import fastmatch_amd                                   # noqa: F401
from fastmatch_amd import fastmatch, cache, synth

# "images": 800 x 640 like images/graf, ~3000 keypoints each
q, t = synth.image_pair((800, 640), 3000, seed=1)
query_cache = cache.Metric_Cache.from_arrays(q["descriptors"], q["positions"], q["size"],
                                             q["thumb_descriptors"], q["thumb_positions"], q["thumb_size"])
target_img = cache.Feature_Image(t["size"], t["positions"], t["descriptors"],
                                 t["thumb_positions"], t["thumb_descriptors"], t["thumb_size"])

log = []                                               # per-round log as figures.visualize_log consumes it
options = {"log": log}                                 # a log forces the host-driven loop; drop it for the device loop
match_fun = fastmatch.match(query_cache, target_img, options)
matches = match_fun(0.7)

print("%d matches in %d rounds" % (len(matches), len(log)))
index, info = matches[0]
print("first match: query keypoint %d at %s -> target %s, ratio %.3f"
      % (index, info["positions"][0], info["positions"][1], info["ratio"]))
planted = q["planted"]
good = sum(1 for i, m in matches
           if planted[i] >= 0 and np.allclose(m["positions"][1], t["positions"][planted[i]], atol=1e-9))
print("%d of them are planted correspondences" % good)
fast = fastmatch.match(query_cache, target_img, {})(0.7)          # same result from the device-resident loop
assert [m[0] for m in fast] == [m[0] for m in matches]

# The reference's evaluation asks one pair for a whole list of thresholds (turntable.py:59-60): a list goes
# through ONE launch of the device loop, one workgroup per threshold.
taus = [0.5, 0.6, 0.7, 0.8, 0.9]
per_tau = fastmatch.match(query_cache, target_img, {})(taus)
print("matches per threshold:", dict(zip(taus, (len(m) for m in per_tau))))
assert [m[0] for m in per_tau[2]] == [m[0] for m in matches]

# Retrieval: which image of a database does a query match?  cv2.BFMatcher's train collection (add / train) on the device:
# one call searches all images, and the per-image ratio test votes for the image that holds the query's object.
from fastmatch_amd import matchutil                                # noqa: E402
rng = np.random.default_rng(3)
database = [synth.synth_sift(1500, rng) for _ in range(20)]       # twenty unrelated images ...
database[13][:400] = q["descriptors"][:400]                        # ... one of them sees a part of the query image
matcher = matchutil.BFMatcher(matchutil.NORM_L2)
matcher.add(database)
votes = matcher.votes(q["descriptors"], 0.8, mode=1)               # query rows passing Lowe's test inside each image
print("retrieval: image %d wins with %d votes (runner-up %d)" % (votes.argmax(), votes.max(), np.sort(votes)[-2]))
assert votes.argmax() == 13 and matcher.match(q["descriptors"][:400])[0].imgIdx == 13

# Fast-Match's own acceptance test against the database, image by image: (q, t) is kept when t is q's cross-checked nearest
# neighbour inside the image and dist(q, t) / selfdist(q) < tau.  One call, one list of DMatch per image.
three = [database[13], database[2], database[7]]
fm_matcher = matchutil.BFMatcher(matchutil.NORM_L2)
fm_matcher.add(three)
per_image = fm_matcher.fastMatchEach(q["descriptors"], 0.7)
print("fast-match acceptance per image:", [len(l) for l in per_image])
assert len(per_image[0]) >= 390 > max(len(per_image[1]), len(per_image[2])) and all(d.imgIdx == 0 for d in per_image[0])

# The match graph of structure from motion and stitching: the images of a set against EACH OTHER, every pair in one call
# (pairs=None: every a < b; a list of (a, b) runs a sliding window or the pairs a retrieval step chose).
views = [synth.synth_sift(800, rng) for _ in range(6)]
views[4][:300] = views[1][100:400]                                 # images 1 and 4 see the same object
graph = matchutil.BFMatcher(matchutil.NORM_L2)
graph.add(views)
edges = graph.matchPairs(ratio=0.8, symmetric=True)                # {(a, b): [DMatch]}, mutual nearest neighbours + ratio test
best = max(edges, key=lambda ab: len(edges[ab]))
print("match graph: %d pairs, the strongest edge %s has %d matches" % (len(edges), best, len(edges[best])))
assert len(edges) == 15 and best == (1, 4) and len(edges[best]) >= 290 and all(d.imgIdx == 4 for d in edges[best])

# Wide float descriptors: a learned extractor's 256-D rows (SuperPoint and its kin) go the same way -- a float array of
# 129 .. 256 columns becomes a wide float bank; k <= 2, crossCheck, the ratio match and the mutual ratio match take it.
wide_t = rng.standard_normal((2000, 256)).astype(np.float32)
wide_t /= np.linalg.norm(wide_t, axis=1, keepdims=True)
wide_q = wide_t[:500] + np.float32(0.01) * rng.standard_normal((500, 256)).astype(np.float32)
qidx, tidx, dist, ratio = matchutil.mutual_ratio_match_arrays(wide_q, wide_t, 0.8)
print("256-D pair: %d of 500 query rows matched mutually at ratio 0.8" % len(qidx))
assert np.array_equal(qidx, tidx) and len(qidx) == 500

# ... and so does their match graph: wide images enter a collection through add_wide, matchPairs is the call it was.
wide_views = [wide_t[300 * i:300 * i + 400].copy() for i in range(4)]      # neighbouring views share 100 rows
wide_graph = matchutil.BFMatcher(matchutil.NORM_L2)
wide_graph.add_wide(wide_views)
wide_edges = wide_graph.matchPairs(ratio=0.8, symmetric=True)
print("256-D match graph: %d pairs, (0, 1) has %d matches, (0, 2) has %d" % (len(wide_edges), len(wide_edges[(0, 1)]), len(wide_edges[(0, 2)])))
assert len(wide_edges) == 6 and len(wide_edges[(0, 1)]) == 100 and len(wide_edges[(0, 2)]) == 0

# Binary descriptors (ORB, 32 bytes): a distance threshold instead of k -- every database row within 40 bits of a query row.
# Distances are integers and the compare is strict, so "h <= 40" is maxDistance = 40.5.
orb_db = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
orb_q = orb_db[:200].copy()
orb_q[:, 0] ^= 0b10110                                             # the same rows, three bits flipped
near = matchutil.hamming_radius_match(orb_q, orb_db, 40.5)
print("ORB radius match: %d of 200 query rows found within 40 bits, %d entries in all" % (sum(bool(l) for l in near), sum(map(len, near))))
assert all(l and l[0].trainIdx == i and l[0].distance == 3.0 for i, l in enumerate(near))

# Fast-Match's own test on the same ORB rows: the cross-checked nearest neighbour is accepted while its distance is small
# beside the query row's distance to its nearest OTHER query row (the Hamming self distance, computed on the device).
# A query row with a duplicate has self distance 0 and is never accepted: rows 3 and 7 here.
orb_q[7] = orb_q[3]
accepted = matchutil.hamming_fast_match(orb_q, orb_db, 0.5)
print("ORB Fast-Match: %d of 200 query rows accepted at tau 0.5" % len(accepted))
assert sorted(m.queryIdx for m in accepted) == [i for i in range(200) if i not in (3, 7)]
assert all(m.trainIdx == m.queryIdx and m.distance == 3.0 for m in accepted)
