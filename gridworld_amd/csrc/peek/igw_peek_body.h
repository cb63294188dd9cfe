// igw_peek_body.h -- the statements of the peek kernel, one copy: block = (env, chunk of 64 candidates).  Included INSIDE the
// body of each __global__ entry (igw_peek_kernel, igw_peek_dict_kernel<FLY>), which names its policy `Space` and its
// parameters `p` (Params<Space::Actions>); everything it calls is igw_peek_core.h's.  Text, not a function template: a
// callee is optimised on its own and once more after it is inlined, and that second round moved instructions of these
// register-bound kernels (measured: walking Dict 0.25 % slower); as text the code objects are the ones of the two files
// this replaces, instruction for instruction.  No include guard, on purpose.
    __shared__ Shared sh;
    const Grp<4> G;
    const int tid = (int)threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int64_t bid = (int64_t)blockIdx.x;
    const int64_t env = bid / p.chunks;
    const int chunk = (int)(bid - env * p.chunks);
    const int slot = tid >> 2;
    const bool real = chunk * kCand + slot < p.K;
    const int k = real ? chunk * kCand + slot : p.K - 1;   // (a candidate past K plays the last one's actions and stores nothing)
    const bool writer = real && G.gl == 0;

    // ---- the env: records, task, live rows
    Env e;
    const int64_t task = (int64_t)__builtin_amdgcn_readfirstlane(env_load(e, p.agent + env, p.aux + env));
    const bool has_start = __builtin_amdgcn_readfirstlane((int)gload(&p.task_meta[task].has_start)) != 0;
    const int8_t* grid_g = p.grid + env * STRIDE;
    const int8_t* start_g = p.task_start + task * STRIDE;
    uint32_t* occ_s = sh.occ[slot];
    for (int w = G.gl; w < OCC_PITCH; w += 4) {   // words 0..15 and 64..71 constant (occ_const_word), 16..63 the env's
        const bool var = (w >= OCC_VAR0) & (w < OCC_VAR0 + OCC_WORDS);
        occ_s[w] = var ? gload(p.occ + env * OCC_WORDS + (var ? w - OCC_VAR0 : 0)) : occ_const_word(w);
    }
    if (tid < WAVE) reinterpret_cast<uint4*>(sh.hist)[tid] = gload(reinterpret_cast<const uint4*>(p.hist + env * HIST_ROW) + tid);
    else if (tid < WAVE + IGW_TASK_INDEX_BYTES / 16)
        reinterpret_cast<uint4*>(sh.index)[tid - WAVE] =
            gload(reinterpret_cast<const uint4*>(p.task_index + task * IGW_TASK_INDEX_BYTES) + (tid - WAVE));
    __syncthreads();

    TrigCtx trig;
    // sincos_deg<true> reads lut[2 * k] = cos and lut[2 * k + 1] = sin of entry k < IGW_LUT_N: the host table's layout
    static_assert(sizeof(IGW_TRIG_LUT_HOST) == sizeof(double) * 2 * IGW_LUT_N, "the trig table is IGW_LUT_N (cos, sin) pairs of doubles");
    trig.lut = &IGW_TRIG_LUT_HOST[0][0];   // a const table with a constant initialiser: constant memory of this code object

    const int64_t row = env * p.K + k;                                   // the candidate's row of the outputs
    const auto act0 = Space::first(p.act, (p.per_env ? row : (int64_t)k) * p.H);   // ... and its first action
    uint32_t* const scratch = sh.wscr[wave];
    bool live = true;
    int ends = 0, nch = 0;
    double ret = 0.0, g = 1.0;
    for (int h = 0; h < p.H; h++) {
        CellChange ch;
        ch.idx = -1; ch.old_val = ch.new_val = 0;
        int size_new = e.prev_size;
        if (live) {
            const Act w = Space::parse(p.act, act0, h);
            e.step_no = min(e.step_no + 1, 65535);  // env.py:276
            Motion mv;
            const ActPre ap = world_act_pre<Space>(G, p.select_and_place, e, trig, w, mv);
            Hit hit;
            hit.hit = false; hit.have_prev = false;
            hit.bx = hit.by = hit.bz = hit.px = hit.py = hit.pz = 0;
            if (ap.want_sight) hit = hit_test<4>(G, occ_s, e.x, e.y, e.z, ap.vx, ap.vy, ap.vz, false, scratch);
            ch = world_act_post(G, e, occ_s, sh.list, slot, nch, grid_g, ap, hit);
            int start_val = 0;
            if (ch.idx >= 0) {
                if (has_start) start_val = (int)gload(start_g + ch.idx);
                if (G.gl == 0)
                    sh.list[nch][slot] = (uint32_t)ch.idx | (uint32_t)ch.new_val << 11 | (uint32_t)(uint8_t)ch.old_val << 16 |
                                         (uint32_t)(uint8_t)start_val << 24;
                nch++;   // (at most one per step: nch <= H <= kMaxH)
            }
            world_update<Space>(G, e, occ_s, mv);
            finish_break(e, ch);
            size_new = e.prev_size + syn_size_delta(ch, start_val);  // synthetic grid = grid - start (env.py:290)
        }
        // ---- max_int = maximal_intersection(grid) where wrong_placement != 0 (tasks/task.py:112): the live row with all
        // of the candidate's changes, one candidate of the wavefront after the other
        const bool need = live && size_new != e.prev_size;
        int mi = e.max_int;
        uint64_t todo = __ballot(need && G.gl == 0);
        while (todo != 0) {   // at most kCandWave rounds
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int cw = l >> 2, cs = wave * kCandWave + cw;
            const int n_c = __builtin_amdgcn_readlane(nch, l);
            wave_sync();
            reinterpret_cast<uint4*>(scratch)[G.lane] = reinterpret_cast<const uint4*>(sh.hist)[G.lane];
            wave_sync();
            for (int i = 0; i < n_c; i++) {
                const uint32_t ent = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.list[i][cs]);
                const int st = (int)(int8_t)(ent >> 24);
                vote_change(scratch, sh.index, (int)(ent & 0x7ffu), (int)(int8_t)((ent >> 16) & 0xffu) - st, (int)((ent >> 11) & 15u) - st);
            }
            wave_sync();
            const int best = wave_max_nonneg(row_piece_max(reinterpret_cast<const uint4*>(scratch)[G.lane]));
            if ((G.lane >> 2) == cw) mi = best;
        }
        wave_sync();
        float r32 = 0.0f;
        int chg = -1;
        if (live) {
            const StepOut o = finish_step(p, e, size_new, mi);
            ret = ret + g * o.reward;
            g = g * p.gamma;
            r32 = (float)o.reward;
            chg = ch.idx >= 0 ? (ch.idx | ch.new_val << 11) : -1;
            if (o.done) {
                live = false;
                ends = h + 1;
            }
        }
        if (writer) {
            if (p.reward) gstore(p.reward + row * p.H + h, r32);
            if (p.change) gstore(p.change + row * p.H + h, (int16_t)chg);
        }
    }
    if (writer) {
        if (p.ends) gstore(p.ends + row, (int16_t)ends);
        if (p.ret) gstore(p.ret + row, (float)ret);
        if (p.pose) {   // out_piece_step's casts (env.py:281-289)
            float* o = p.pose + row * IGW_PEEK_POSE;
            gstore(o + 0, (float)e.x);
            gstore(o + 1, (float)e.y);
            gstore(o + 2, (float)e.z);
            gstore(o + 3, (float)e.pitch);
            gstore(o + 4, (float)e.yaw);
        }
    }
