// ref_extract_depth_driver.cpp -- TEST INFRASTRUCTURE: the second translation unit of oracle/_ref/libref_sah.so.
// It #includes BottomUpBuilder.cu from the reference tree where it lies, for ExtractDepth, the kernel that hands the
// hybrid build's sub-roots to SharedTaskBuild (BuildWrapper.cu:350-360).  It is a file of its own because
// BottomUpBuilder.cu and SharedTaskBuilder.cu both include DeviceUtils.cuh, which has no include guard; and it is part
// of libref_sah.so, not an entry of ref_kernels_driver.cpp, so that libref_kernels.so is built from exactly the files
// it was built from before and the hybrid comparison needs nothing of it.  threadIdx & co. are ref_sah_driver.cpp's.
//
// ExtractDepth has no barrier and claims its output slots with atomicAdd: it runs serially in tid order, like
// GenerateMortonCodesPairs in ref_kernels_driver.cpp.  That is one arrival order; callers compare the sub-roots as a set.
#include "BottomUpBuilder.cu"

extern "C" {

// ExtractDepth<<<1, 256>>> (BuildWrapper.cu:351-354).  nodes: the finished LBVH.  p_aabb: the scene box as ordered ints,
// converted to floats in place by thread 0; c_aabb: six floats, grown from the caller's empty box.  out_indices: 256
// PrimitiveID {pair slot, 2}; out_aabbs: 256 boxes.  Returns the number of sub-roots.
int ref_extract_depth(void* nodes, void* out_indices, void* out_aabbs, void* c_aabb, void* p_aabb, unsigned root,
                      unsigned target_depth, unsigned count)
{
    int out_count = 0;
    blockDim = dim3(256, 1, 1);
    gridDim = dim3(1, 1, 1);
    blockIdx = make_uint3(0, 0, 0);
    for (unsigned t = 0; t < 256; ++t) {
        threadIdx = make_uint3(t, 0, 0);
        ExtractDepth((Node*)nodes, (PrimitiveID*)out_indices, (AABB*)out_aabbs, &out_count, (AABB*)c_aabb,
                     (AABB*)p_aabb, root, target_depth, count);
    }
    return out_count;
}

}  // extern "C"
