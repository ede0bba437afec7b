    // rt_ray_first_body.inc -- the body of a first-K ray kernel (rt_ray_first.hpp says who includes it and what they define).
    // the counters' workgroup sums reuse the stack's LDS once every lane is done with it (no extra bytes)
    __shared__ alignas(8) RfEntry stack_lds[kTraceWaves][kRfStackLds][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t vb = xcd_chunk_block(blockIdx.x, gridDim.x);
    const uint64_t i = ((uint64_t)vb * kTraceWaves + (uint32_t)wave) * 64u + (uint32_t)lane;
    const bool in_range = i < p.num_rays;
    const uint32_t k = p.k;

    float4 ra = {0.f, 0.f, 0.f, 0.f}, rb = {0.f, 0.f, 0.f, -1.f};
    if (in_range) { ra = p.rays[2 * i]; rb = p.rays[2 * i + 1]; }
    Ray r;
    r.ox = ra.x; r.oy = ra.y; r.oz = ra.z; r.tmin = ra.w;
    r.dx = rb.x; r.dy = rb.y; r.dz = rb.z; r.tmax = rb.w;
    r.ix = 1.0f / r.dx; r.iy = 1.0f / r.dy; r.iz = 1.0f / r.dz;
    const float tmax0 = r.tmax;
    // not traced (a row of misses, no tests), rt_intersect_rays's rule: lanes past the batch, an empty or NaN [tmin, tmax], a
    // NaN origin or direction
    const bool nan_ray = __builtin_isnan(r.ox) | __builtin_isnan(r.oy) | __builtin_isnan(r.oz) | __builtin_isnan(r.dx) |
                         __builtin_isnan(r.dy) | __builtin_isnan(r.dz);
    bool live = in_range && r.tmin <= r.tmax && !nan_ray && p.count > 0;
    const RT_BODY_FILTER flt = RT_BODY_MAKE_FILTER(i, in_range);

    // the list: m records in ascending (t, id) order.  Only a live lane touches it, and a live lane is in range.
    float4 list[RT_RAY_FIRST_MAX_K];
    uint32_t m = 0;
    float kth_t = __builtin_inff();   // the k-th record, valid once m == k
    uint32_t kth_id = RT_MISS;
    float bound = tmax0;              // tmax while m < k (or while the k-th t is NaN), kth_t after

    lds_rf_entry* const col = (lds_rf_entry*)&stack_lds[wave][0][lane];
    RfSpill spill;
    int sp = 0;
    bool overflow = false;            // a push was dropped: the row is a subset
    uint32_t box_tests = 0, tri_tests = 0;
    uint32_t cur = (p.root & kIndexMask) | (p.count << 29);

    // an accepted triangle (t <= bound, stored weights bu / bv, rotation rot)
    auto offer = [&](float t, uint32_t id, float bu, float bv, uint32_t rot) {
        const bool full = m == k;
        if (full && !rf_below(t, id, kth_t, kth_id)) return;                  // not below the k-th: registers only
        // the position: the records above the candidate are [pos, m); a full list's k-th is above it (the test before)
        const uint32_t top = full ? k - 1 : m;
        uint32_t pos = top;
        while (pos > 0) {
            const float4 e = list[pos - 1];
            const uint32_t eid = __float_as_uint(e.y);
            if (rf_same_t(e.x, t) && eid == id) return;                       // already listed
            if (rf_below(e.x, eid, t, id)) break;
            pos--;
        }
        // the shift, from the top down: [pos, top) -> [pos + 1, top + 1); a full list loses its k-th
        for (uint32_t j = top; j > pos; j--) list[j] = list[j - 1];
        // RotateAttributes, as ray_query_kernel: leaf corner k is the caller's corner i_k
        const float w0 = 1 - bu - bv;
        float4 o;
        o.x = t;
        o.y = __uint_as_float(id);
        o.z = rot == 1 ? bv : (rot == 2 ? w0 : bu);
        o.w = rot == 1 ? w0 : (rot == 2 ? bu : bv);
        list[pos] = o;
        m = top + 1;
        if (m == k) {
            if (pos == k - 1) { kth_t = t; kth_id = id; }
            else { const float4 e = list[k - 1]; kth_t = e.x; kth_id = __float_as_uint(e.y); }
            bound = __builtin_isnan(kth_t) ? tmax0 : kth_t;
        }
    };
    // one triangle (leaf corners c0, c1, c2, rotation rot) against [tmin, bound]
    auto test = [&](float c0x, float c0y, float c0z, float c1x, float c1y, float c1z, float c2x, float c2y, float c2z,
                    uint32_t prim, uint32_t rot) {
        Hit h;
        if (intersect_tri(c0x, c0y, c0z, c1x, c1y, c1z, c2x, c2y, c2z, r, h, 0u, prim, flt)) offer(r.tmax, prim, h.bu, h.bv, rot);
        r.tmax = bound;               // intersect_tri shrank it to t: the window's end is the bound, nothing else
    };
    auto next_from_stack = [&]() {
#if RT_RAY_FIRST_PENDING == 8
        while (sp > 0) {              // re-culled against the current bound, never on equality
            --sp;
            const RfEntry se = sp < kRfStackLds ? col[sp * 64] : spill[sp - kRfStackLds];
            if (__uint_as_float((uint32_t)(se >> 32)) <= bound) { cur = (uint32_t)se; return; }
        }
        live = false;
#else
        if (sp == 0) { live = false; return; }
        --sp;
        cur = sp < kRfStackLds ? col[sp * 64] : spill[sp - kRfStackLds];
#endif
    };
    auto leaf_step = [&]() {
        tri_tests++;
        const uint4* tp = reinterpret_cast<const uint4*>(p.leaves + (cur & kIndexMask));
        uint4 l0 = tp[0], l1 = tp[1], l2 = tp[2], l3 = tp[3];
        // all sixteen dwords are "used" here: the four loads stay four 16-byte requests issued together (rt_traverse.hpp)
        asm volatile("" : "+v"(l0.x), "+v"(l0.y), "+v"(l0.z), "+v"(l0.w), "+v"(l1.x), "+v"(l1.y), "+v"(l1.z), "+v"(l1.w),
                          "+v"(l2.x), "+v"(l2.y), "+v"(l2.z), "+v"(l2.w), "+v"(l3.x), "+v"(l3.y), "+v"(l3.z), "+v"(l3.w));
        test(__uint_as_float(l0.x), __uint_as_float(l0.y), __uint_as_float(l0.z),
             __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
             __uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z), l0.w, l2.w & 0xFFFFu);
        // triangle B = (v2, v1, v3); for a single triangle v3 == v2 bit for bit and B is skipped (as trace_ray)
        if (l3.x != l2.x || l3.y != l2.y || l3.z != l2.z)
            test(__uint_as_float(l2.x), __uint_as_float(l2.y), __uint_as_float(l2.z),
                 __uint_as_float(l1.x), __uint_as_float(l1.y), __uint_as_float(l1.z),
                 __uint_as_float(l3.x), __uint_as_float(l3.y), __uint_as_float(l3.z), l1.w, l2.w >> 16);
        next_from_stack();
    };
    auto box_step = [&]() {
        const uint32_t first = cur & kIndexMask, cnt = cur >> 29;
        uint32_t near_e = kNoNear;
        float near_f = __builtin_inff();
        for (uint32_t s = 0; s < cnt; s++) {
            const uint4* np = reinterpret_cast<const uint4*>(p.nodes + first + s);
            const uint4 a = np[0], b = np[1];
            const uint32_t type = b.w >> 29;
            if (type == RT_CHILD_NONE) continue;
            box_tests++;
            const uint32_t e = slot_entry(a, b);
            float front, back;
            slab(a, b, r, front, back);
            const bool in = (back >= front) & (front <= bound) & (back >= r.tmin);
            if (!in || (type != RT_CHILD_TRI && (e >> 29) == 0)) continue;   // missed or pruned, or an empty run
            uint32_t pe = e;
            float pf = front;
            if (front < near_f) {             // the new nearest; the old one (if any) is pushed
                pe = near_e; pf = near_f;
                near_e = e; near_f = front;
            }
            if (pe != kNoNear) {
#if RT_RAY_FIRST_PENDING == 8
                const RfEntry se = (uint64_t)pe | ((uint64_t)__float_as_uint(pf) << 32);
#else
                const RfEntry se = pe;
                (void)pf;
#endif
                if (sp < kRfStackLds) col[sp * 64] = se;
                else if (sp < kStackMax) spill[sp - kRfStackLds] = se;
                else overflow = true;         // dropped: what lies below it is missing from the row
                sp = min(sp + 1, kStackMax);
            }
        }
        if (near_e != kNoNear) cur = near_e;
        else next_from_stack();
    };

    while (true) {
        uint64_t stepping, parked;
        while (true) {                        // box phase: step while enough lanes hold a box run
            stepping = __builtin_amdgcn_ballot_w64(live && (cur >> 29) != 0);
            parked = __builtin_amdgcn_ballot_w64(live && (cur >> 29) == 0);
            if (stepping == 0 || __popcll(stepping) * kParkDen < __popcll(parked) * kParkNum) break;
            if (live && (cur >> 29) != 0) box_step();
        }
        if ((stepping | parked) == 0) break;
        if (live && (cur >> 29) == 0) leaf_step();   // leaf phase: every lane that holds a leaf
    }

    if (in_range) {
        float4* const row = p.out + i * k;
        const float4 miss = {__builtin_inff(), __uint_as_float((uint32_t)RT_MISS), 0.0f, 0.0f};
        for (uint32_t j = 0; j < k; j++) row[j] = j < m ? list[j] : miss;
    }
    if (p.status && __builtin_amdgcn_ballot_w64(overflow) != 0 && lane == 0)
        atomicOr(p.status, (uint32_t)RT_RAY_FIRST_STACK_OVERFLOW);
    if (p.counters) {                         // (kernel argument: the same for every thread)
        const uint32_t bsum = wave_sum_u32(box_tests), tsum = wave_sum_u32(tri_tests);
        unsigned long long* const csum = reinterpret_cast<unsigned long long*>(&stack_lds[0][0][0]);
        __syncthreads();                      // every lane is done with its stack column
        if (threadIdx.x < 2) csum[threadIdx.x] = 0ull;
        __syncthreads();
        if (lane == 0) {
            atomicAdd(&csum[0], (unsigned long long)bsum);
            atomicAdd(&csum[1], (unsigned long long)tsum);
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            const unsigned long long v = csum[threadIdx.x];
            if (v) atomicAdd(&p.counters[threadIdx.x], v);
        }
    }
