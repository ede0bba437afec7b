    // rt_instance_query_body.inc -- the body of an instanced ray query kernel<PF, ANY>(InstParams p, ...): ray setup, the
    // two-level traversal, the record and instance id of the hit, the per-workgroup counters.  Included as TEXT inside the braces
    // of instance_query_kernel (instances.hip) and instance_query_filtered_kernel (instance_filter_query.hip), which define
    // RT_BODY_MAKE_FILTER(i, in_range): the expression that makes lane i's instance-filter policy for trace_instanced
    // (rt_instance_traverse.hpp).  Text, not a function template: called from the kernel the body comes out a line or two
    // different in the unfiltered instantiations (DESIGN sections 20 and 21).
    __shared__ uint32_t stack_lds[kTraceWaves][kStackLds][64];
    __shared__ unsigned long long csum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (p.counters) {
        if (threadIdx.x < 4) csum[threadIdx.x] = 0ull;
        __syncthreads();
    }
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_rays;

    Ray r;
    r.ox = r.oy = r.oz = r.dx = r.dy = r.dz = r.ix = r.iy = r.iz = 0.0f;
    r.tmin = 0.0f;
    r.tmax = -1.0f;
    if (in_range) {
        load_world_ray(p, i, r);
        r.tmin = p.rays[2 * i].w;
        r.tmax = p.rays[2 * i + 1].w;
    }
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    const bool active = in_range && r.tmin <= r.tmax && !nan_ray;

    SpillArray spill;
    Trav t;
    t.lds = (lds_u32*)&stack_lds[wave][0][lane];
    t.spill = spill;
    uint32_t steps[2] = {0u, 0u};
    Hit h = {0u, 0u, 0.f, 0.f};
    uint32_t hit_inst = RT_MISS;
    const bool hit = trace_instanced<PF, ANY>(p, i, r, h, hit_inst, t, active, steps, RT_BODY_MAKE_FILTER(i, in_range));

    if (in_range) {
        float4 o = {__builtin_inff(), __uint_as_float(RT_MISS), 0.f, 0.f};
        if (hit) {
            // the hit instance's BLAS leaves; (u, v) back to the caller's corners as ray_query_kernel does
            const uint32_t b = reinterpret_cast<const uint4*>(p.records + hit_inst)[3].x;
            const rt_triangle_pair* lv = reinterpret_cast<const rt_triangle_pair*>(
                *reinterpret_cast<const uint64_t*>(p.blas_table + b));
            const uint32_t rot = lv[h.tri_id >> 1].rotations[h.tri_id & 1];
            const float w0 = 1 - h.bu - h.bv;
            o.x = r.tmax;
            o.y = __uint_as_float(h.primitive_id);
            o.z = rot == 1 ? h.bv : (rot == 2 ? w0 : h.bu);
            o.w = rot == 1 ? w0 : (rot == 2 ? h.bu : h.bv);
        }
        p.hits[i] = o;
        p.instance_ids[i] = hit ? hit_inst : RT_MISS;
    }
    if (p.counters) {
        const uint32_t bsum = wave_sum_u32(t.box_tests), tsum = wave_sum_u32(t.tri_tests);
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
            atomicAdd(&csum[2], (unsigned long long)steps[0]);
            atomicAdd(&csum[3], (unsigned long long)steps[1]);
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&p.counters[threadIdx.x], v);
        }
    }
