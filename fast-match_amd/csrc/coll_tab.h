// A train collection's device lookup tables (api_collection.hip builds them in fm_collection_train) and the lookup every
// kernel that reports a row of the stack shares: the merge / translate kernels of api_collection.hip, K10's compaction
// (radius.hip).  Per 128-row stage: its image and its number of real rows; per image: its first physical row.
#pragma once
#include <cstdint>

namespace fm {

struct CollTab { const int32_t* st_img; const int32_t* st_real; const int32_t* img_phys; };

// physical row of the stack -> (image, row inside it); false for a padding row
__device__ __forceinline__ bool coll_lookup(const CollTab& t, unsigned p, int32_t& img, int32_t& local)
{
    const unsigned s = p >> 7;
    if ((int)(p & 127u) >= t.st_real[s]) return false;
    img = t.st_img[s];
    local = (int32_t)(p - (unsigned)t.img_phys[img]);
    return true;
}

__device__ __forceinline__ bool coll_real(const CollTab& t, unsigned long long key)
{
    return key != ~0ull && (int)((unsigned)key & 127u) < t.st_real[(unsigned)key >> 7];
}

}  // namespace fm
