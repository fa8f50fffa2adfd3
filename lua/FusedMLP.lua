-- lua/FusedMLP.lua -- the DEVICE-RESIDENT form of mlp.lua's step for MI355X: what replaces `mlp:run` when the
-- minibatch is to stay in HBM from the input packer to the gradients (the module-level lua/VBLinear.lua keeps
-- mlp.lua unchanged but crosses PCIe at every module). Same protocol as the reference's mlp.lua --
--     mlp:resetGradients()  (mlp.lua:62-67)      mlp:sample()   (:69-74)      mlp:run(inputs, targets)  (:76-84)
--     mlp:calc_lc(opt)      (:109-115)           mlp:update(opt) (:117-142)
-- -- over the C ABI of include/vbnn_hip.h, call for call the sequence of vbnn_amd/engine.py:FusedMLP (run: lines
-- "forward" / "fused classifier head" / "backward"), which is what the GPU parity tests execute. LRT mode, total
-- gradients from the accGradParameters epilogue (VBLinear.lua:90-98 folded in), S draws accumulate in place.
-- Data-parallel: one process per GPU; `opt.world` / `opt.rank` / `opt.comm_id` (the 128 bytes of
-- vbnn_comm_unique_id, handed to every rank by the launcher) switch on the RCCL exchange of the gradient buckets.
--
-- NOT EXECUTED in the build image (no LuaJIT / Torch7 there). Its executable stand-in is tools/c_host.c: the same
-- functions (new / _alloc_batch / prepare / run / update), the same library calls in the same order, in plain C over the
-- same header, run on the GPU by tests/test_c_host.py and bitwise equal to engine.py there. tests/test_abi.py and
-- tests/test_c_host.py lint this file structurally: every C.vbnn_* it calls is declared in the header with that many
-- parameters, every struct field it sets exists, and the call ORDER of each function is the C host's and engine.py's.
local vb = require('vbnn_ffi')
local ffi, C, check = vb.ffi, vb.C, vb.check

local FusedMLP = {}
FusedMLP.__index = FusedMLP

local function f32(p) return ffi.cast('float*', p) end
local function packed(rows, cols, esize)
    local ld = vb.pad_ld(cols)
    return { p = vb.alloc(rows * ld * esize), ld = ld, rows = rows }
end

-- opt: input_size, hidden = {..}, n_classes (<= 16: the fused classifier head), var_init, B, S, seed, dtype ('bf16')
function FusedMLP.new(opt)
    local self = setmetatable({}, FusedMLP)
    self.opt = opt
    self.dtype = (opt.dtype == 'f32') and C.VBNN_F32 or C.VBNN_BF16
    self.esize = (self.dtype == C.VBNN_BF16) and 2 or 4
    self.seed, self.B, self.S = opt.seed or 3, opt.B, opt.S or 1
    self.world, self.rank = opt.world or 1, opt.rank or 0
    -- opt.kl_in_update (default: true for bf16, as engine.py): the gradient arena holds the LIKELIHOOD parts and update() adds the
    -- exact fp32 KL gradient (vbnn_update_desc.kl_add); false = the KL part fused into the accGradParameters epilogue (A/B)
    if opt.kl_in_update == nil then self.kl_in_update = (self.dtype == C.VBNN_BF16) else self.kl_in_update = opt.kl_in_update end
    -- opt.exchange_mode = 'sharded' (data-parallel, bf16): the sharded-update exchange instead of the all-reduce -- reduce-scatter of the
    -- gradients by layer rows, update() on this rank's rows, all-gather of the operand shadows + statistics (INTEGRATION.md section 4)
    self.sharded = opt.exchange_mode == 'sharded'
    if self.sharded then
        assert(opt.comm_id and self.dtype == C.VBNN_BF16, "exchange_mode = 'sharded': data-parallel (comm_id), bf16")
        self.kl_in_update = true
    end
    self.n_classes = opt.n_classes
    assert(self.n_classes <= 16, 'FusedMLP.lua drives the fused classifier head (mlp.lua:29-32); see engine.py for wider ones')
    local sizes = { opt.input_size }
    for _, h in ipairs(opt.hidden) do sizes[#sizes + 1] = h end
    self.sizes = sizes
    -- gradient arena: [d/dlvars | d/dmeans | d/dbias] per VB layer, then the final Linear (vbnn_amd/partition.py)
    local total = 0
    for li = 1, #sizes - 1 do total = total + 2 * sizes[li] * sizes[li + 1] + sizes[li + 1] end
    total = total + sizes[#sizes] * self.n_classes + self.n_classes
    self.n_grads = total
    self.grads = vb.alloc(total * 4)
    local off = 0
    local function take(n) local p = f32(self.grads) + off; off = off + n; return p end
    self.vb = {}
    for li = 1, #sizes - 1 do
        local I, O = sizes[li], sizes[li + 1]
        local v = { I = I, O = O, layer_id = li - 1, bucket_off = off }
        v.means, v.lvars, v.bias = vb.alloc(O * I * 4), vb.alloc(O * I * 4), vb.alloc(O * 4)
        v.m_mu, v.v_mu, v.m_lv, v.v_lv = vb.alloc(O * I * 4), vb.alloc(O * I * 4), vb.alloc(O * I * 4), vb.alloc(O * I * 4)
        v.grad_lv, v.grad_mu, v.gradBias = take(O * I), take(O * I), take(O)
        v.bucket_n = off - v.bucket_off
        v.stats = vb.alloc(32)
        v.mu_s, v.var_s = packed(O, I, self.esize), packed(O, I, self.esize)
        if li > 1 then v.muT_s, v.varT_s = packed(I, O, self.esize), packed(I, O, self.esize) end
        v.use_muT = li > 1                                        -- until _alloc_batch has asked the library (K-major weights)
        v.t = 0
        -- VBLinear.lua:18,22-28 + the He rule of mlp.lua:47-55 for the means (stream 5 = VBNN_STREAM_HEINIT)
        check(C.vbnn_fill_normal(vb.ctx, f32(v.means), O, I, I, self.seed, 5, v.layer_id, 0, 0, math.sqrt(2 / I)))
        local lv0 = torch.FloatTensor(O * I):fill(math.log(opt.msr_init and 2 / I or opt.var_init))
        check(C.vbnn_buf_upload(vb.ctx, v.lvars, lv0:data(), O * I * 4))
        self.vb[li] = v
    end
    local H = sizes[#sizes]
    self.weight3, self.bias3 = vb.alloc(self.n_classes * H * 4), vb.alloc(self.n_classes * 4)
    self.gradWeight3, self.gradBias3 = take(self.n_classes * H), take(self.n_classes)
    check(C.vbnn_fill_normal(vb.ctx, f32(self.weight3), self.n_classes, H, H, self.seed, 5, #self.vb, 0, 0, math.sqrt(2 / H)))
    self.w3_s = packed(self.n_classes, H, self.esize)
    self.acc, self.corr = vb.alloc(16), vb.alloc(4)
    self.draw, self.first = 0, true
    if opt.device_draw then self.draw_dev = ffi.cast('uint32_t*', vb.alloc(4)) end   -- the draw counter on the device
    if self.world > 1 then                                        -- the exchange (include/vbnn_hip.h: vbnn_comm_*)
        local box = ffi.new('vbnn_comm*[1]')
        check(C.vbnn_comm_create(vb.ctx, self.rank, self.world, opt.comm_id, box))
        self.comm = ffi.gc(box[0], C.vbnn_comm_destroy)
    end
    -- single GPU, layers of different sizes: every updateGradInput first, then the accGradParameters from the first layer
    -- up, so that the heavy launches alternate with lighter ones (engine.py: dx_first; the chip is power-bound in them)
    local wmin, wmax = math.huge, 0
    for k = 1, #sizes - 1 do
        wmin, wmax = math.min(wmin, sizes[k] * sizes[k + 1]), math.max(wmax, sizes[k] * sizes[k + 1])
    end
    self.dx_first = (not self.comm) and (2 * wmin <= wmax)
    -- the chained backward launch (engine.py: chain_backward; bf16 without an exchange): updateGradInput's tile first where dx_first
    -- holds, else off; opt.chain_backward = 'dx' / 'dw' / false overrides
    local chain = opt.chain_backward
    if chain == nil then chain = self.dx_first and 'dx' or false end
    self.chain = (self.dtype == C.VBNN_BF16 and not self.comm) and chain or nil
    self:prepare()
    return self
end

-- buffers that depend on the local batch size (engine.py:_alloc_batch; tools/c_host.c:fm_alloc_batch)
function FusedMLP:_alloc_batch(N)
    if self.N == N then return end
    self.N = N
    local km_ok = self.dtype == C.VBNN_BF16 and self.S == 1
    -- fp32 (the general kernel): the minibatch raw, x.x formed in registers, x / g / mu / sigma^2 K-major, the bias gradient
    -- from a synthetic row of ones (engine.py: f32_direct). Not with an exchange (its two-launch accGradParameters wants x.x)
    self.direct = self.dtype == C.VBNN_F32 and not self.comm
    local need_prepare = false
    local ones, ones_dev = torch.FloatTensor(N):fill(1), vb.alloc(N * 4)
    check(C.vbnn_buf_upload(vb.ctx, ones_dev, ones:data(), N * 4))
    for li, v in ipairs(self.vb) do
        local last = li == #self.vb
        v.bias_from_dw = (v.I % 256 ~= 0) and not last          -- the ones column / row of x: bias gradient from the GEMM
        local km = (km_ok and not self.direct) and C.vbnn_kmajor_supported_dw(v.I, v.O, N, v.bias_from_dw and 1 or 0) or 0
        v.dw_km = km > 0 or self.direct
        -- the two-launch form of accGradParameters (early d/dlvars message) needs either the transposed operands or the
        -- plain K-major launch of the two-pass kernel; the few-tile K-major launches compute both GEMMs in one grid
        v.early_ok = (not self.direct) and ((not v.dw_km) or ((not v.bias_from_dw) and C.vbnn_kmajor_supported(v.I, v.O, N) ~= 0))
        v.dx_km = li > 1 and (self.direct or (km_ok and C.vbnn_kmajor_supported(v.I, N, v.O) ~= 0))
        local use_muT = li > 1 and not v.dx_km
        if use_muT and not v.use_muT then need_prepare = true end
        v.use_muT = use_muT
        local extra = v.bias_from_dw and 1 or 0
        local xcols = v.I + (v.dw_km and extra or 0)
        if km == 2 then xcols = math.floor((xcols + 255) / 256) * 256 end
        if self.direct then xcols = v.I end                       -- (the row of ones is synthesised by the kernel)
        v.x_s = packed(N, xcols, self.esize)
        v.x2_s = (not self.direct) and packed(N, xcols, self.esize) or nil
        v.has_t = not v.dw_km                                     -- shapes without a K-major form get the transposed copies
        if v.dw_km and v.bias_from_dw and not self.direct then    -- column I of x is all ones, written once
            check(C.vbnn_pack(vb.ctx, self.dtype, C.VBNN_PACK_COPY, f32(ones_dev), nil, 1, N, 1,
                              ffi.cast('char*', v.x_s.p) + v.I * self.esize, v.x_s.ld, nil, 0))
        end
        if v.has_t then
            v.xT_s, v.x2T_s = packed(v.I + extra, N, self.esize), packed(v.I + extra, N, self.esize)
            v.gT_s, v.gvT_s = packed(v.O, N, self.esize), packed(v.O, N, self.esize)
            if v.bias_from_dw then                                -- row I of x^T is all ones
                check(C.vbnn_pack(vb.ctx, self.dtype, C.VBNN_PACK_COPY, f32(ones_dev), nil, N, 1, N,
                                  ffi.cast('char*', v.xT_s.p) + v.I * v.xT_s.ld * self.esize, v.xT_s.ld, nil, 0))
            end
        end
        v.g_s, v.gv_s = packed(N, v.O, self.esize), packed(N, v.O, self.esize)
        v.r = vb.alloc(N * v.O * self.esize)
    end
    self.h_s = packed(N, self.sizes[#self.sizes], self.esize)
    self.logits, self.out, self.g_logits = vb.alloc(N * self.n_classes * 4), vb.alloc(N * self.n_classes * 4), vb.alloc(N * self.n_classes * 4)
    -- the head's logits from the last VB layer's forward tiles, where that launch can carry them (vbnn_fwd_args.head_slots)
    local vl = self.vb[#self.vb]
    self.n_head_slots = self.draw_dev and 0 or C.vbnn_forward_head_slots(vb.ctx, self.dtype, N, vl.I, vl.O, self.n_classes)
    self.head_slots = self.n_head_slots > 0 and vb.alloc(self.n_head_slots * N * 16 * 4) or nil
    if need_prepare then self:prepare() end
end

function FusedMLP:resetGradients() self.first = true end          -- mlp.lua:62-67: the first draw overwrites

-- VBLinear:compute_prior (VBLinear.lua:77-88) + the operand shadows, once; afterwards vbnn_update maintains both
function FusedMLP:prepare()
    local n = #self.vb
    local d = ffi.new('vbnn_prep_desc[?]', n)
    for k, v in ipairs(self.vb) do
        local e = d[k - 1]
        e.means, e.lvars, e.O, e.I = f32(v.means), f32(v.lvars), v.O, v.I
        e.mu_s, e.var_s, e.ld_w = v.mu_s.p, v.var_s.p, v.mu_s.ld
        e.muT_s, e.varT_s = v.use_muT and v.muT_s.p or nil, v.use_muT and v.varT_s.p or nil
        e.ld_wT = v.muT_s and v.muT_s.ld or 0
        e.stats = ffi.cast('double*', v.stats)
    end
    local w3 = ffi.new('vbnn_pack_desc[1]')
    w3[0].src, w3[0].rows, w3[0].cols, w3[0].ld_src = f32(self.weight3), self.n_classes, self.sizes[#self.sizes], self.sizes[#self.sizes]
    w3[0].dst, w3[0].ld_dst, w3[0].dstT, w3[0].ld_dstT = self.w3_s.p, self.w3_s.ld, nil, 0
    if self.held then check(C.vbnn_prepare_masked(vb.ctx, self.dtype, n, d, self.held, w3))   -- a held pruning mask (:hold_pruned)
    else check(C.vbnn_prepare(vb.ctx, self.dtype, n, d, w3)) end
end

function FusedMLP:sample()                                        -- mlp.lua:69-74: LRT draws its noise in the forward epilogue
    self.draw = self.draw + 1
    if self.draw_dev then check(C.vbnn_sample(vb.ctx, self.draw_dev, 1)) end   -- opt.device_draw: capturable (vbnn_capture_*)
end

-- mlp.lua:76-84, fused. inputs: DEVICE pointer to N x input_size floats (row pitch ld), targets: device int32[N], 0-based
-- sharded-update exchange: layer li's messages after its accGradParameters (tools/c_host.c: fm_scatter)
function FusedMLP:_scatter(li, lv, mu, small)
    local v = self.vb[li]
    local per = v.O * v.I / self.world
    if lv then check(C.vbnn_comm_reduce_scatter(self.comm, f32(self.grads) + v.bucket_off, per)) end
    if mu then check(C.vbnn_comm_reduce_scatter(self.comm, f32(self.grads) + v.bucket_off + v.O * v.I, per)) end
    if small then
        local off = v.bucket_off + 2 * v.O * v.I
        local stop = (li == #self.vb) and self.n_grads or (v.bucket_off + v.bucket_n)
        check(C.vbnn_allreduce_grads(self.comm, f32(self.grads) + off, stop - off))
    end
end

-- the update with the parameters SHARDED by layer rows (tools/c_host.c: fm_update_sharded; engine.py: _update_sharded)
function FusedMLP:_update_sharded(opt)
    local lr = opt.state.learningRate
    local H, G, R, n = self.sizes[#self.sizes], self.world, self.rank, #self.vb
    check(C.vbnn_sgd_step(vb.ctx, f32(self.weight3), self.gradWeight3, self.n_classes * H, lr))
    check(C.vbnn_sgd_step(vb.ctx, f32(self.bias3), self.gradBias3, self.n_classes, lr))
    self.stat_parts = self.stat_parts or vb.alloc(G * n * 4 * 8)
    local parts = ffi.cast('double*', self.stat_parts)
    local mine = parts + R * n * 4
    local d = ffi.new('vbnn_update_desc[?]', n)
    local st = ffi.new('double[4]')
    for k, v in ipairs(self.vb) do
        check(C.vbnn_sgd_step(vb.ctx, f32(v.bias), v.gradBias, v.O, lr))
        v.t = v.t + 1
        local nr = v.O / G
        local r0 = R * nr
        local o = r0 * v.I
        check(C.vbnn_buf_download(vb.ctx, st, v.stats, 32))          -- in: the WHOLE layer's pre-update statistics
        check(C.vbnn_buf_upload(vb.ctx, mine + 4 * (k - 1), st, 32))
        local e = d[k - 1]
        e.means, e.lvars, e.O, e.I = f32(v.means) + o, f32(v.lvars) + o, nr, v.I
        e.mu_s = ffi.cast('char*', v.mu_s.p) + r0 * v.mu_s.ld * self.esize
        e.var_s = ffi.cast('char*', v.var_s.p) + r0 * v.var_s.ld * self.esize
        e.ld_w = v.mu_s.ld
        e.stats, e.grad_mu, e.grad_lv = mine + 4 * (k - 1), v.grad_mu + o, v.grad_lv + o
        e.m_mu, e.v_mu, e.m_lv, e.v_lv = f32(v.m_mu) + o, f32(v.v_mu) + o, f32(v.m_lv) + o, f32(v.v_lv) + o
        for key, cfg in pairs({ mu = opt.meanState, lv = opt.varState }) do
            e[key].lr, e[key].beta1, e[key].beta2 = cfg.learningRate, cfg.beta1 or 0.9, cfg.beta2 or 0.999
            e[key].eps, e[key].lambda, e[key].t = cfg.epsilon or 1e-8, cfg.lambda or 1, v.t
        end
        e.lr_bias, e.B, e.kl_add = lr, self.B, 1
    end
    local w3 = ffi.new('vbnn_pack_desc[1]')
    w3[0].src, w3[0].rows, w3[0].cols, w3[0].ld_src = f32(self.weight3), self.n_classes, H, H
    w3[0].dst, w3[0].ld_dst, w3[0].dstT, w3[0].ld_dstT = self.w3_s.p, self.w3_s.ld, nil, 0
    check(C.vbnn_update(vb.ctx, self.dtype, n, d, w3))
    local stats = ffi.new('double*[?]', n)
    for k, v in ipairs(self.vb) do
        check(C.vbnn_comm_all_gather(self.comm, v.mu_s.p, v.O / G * v.mu_s.ld * self.esize))
        check(C.vbnn_comm_all_gather(self.comm, v.var_s.p, v.O / G * v.var_s.ld * self.esize))
        stats[k - 1] = ffi.cast('double*', v.stats)
    end
    check(C.vbnn_comm_all_gather(self.comm, self.stat_parts, n * 4 * 8))
    check(C.vbnn_comm_finish(self.comm))
    check(C.vbnn_stats_combine(vb.ctx, n, G, parts, stats))
    for _, v in ipairs(self.vb) do
        if v.use_muT then
            check(C.vbnn_transpose_packed(vb.ctx, self.dtype, v.mu_s.p, v.mu_s.ld, v.O, v.I, v.muT_s.p, v.muT_s.ld))
            check(C.vbnn_transpose_packed(vb.ctx, self.dtype, v.var_s.p, v.var_s.ld, v.O, v.I, v.varT_s.p, v.varT_s.ld))
        end
    end
end

function FusedMLP:run(inputs, ld, targets, N)
    self:_alloc_batch(N)
    local accumulate = self.first and 0 or 1
    local inv_n = 1 / (N * self.world)
    local row0 = self.rank * N
    local v0 = self.vb[1]
    for _, v in ipairs(self.vb) do v.x_in, v.ld_in = v.x_s.p, v.x_s.ld end
    if self.direct and ld % 4 == 0 and tonumber(ffi.cast('uintptr_t', inputs)) % 16 == 0 then
        v0.x_in, v0.ld_in = inputs, ld                            -- the GEMMs read the minibatch where it lies: no packing launch
    else
        check(C.vbnn_pack_input(vb.ctx, self.dtype, f32(inputs), ld, N, v0.I, v0.x_s.p, v0.x2_s and v0.x2_s.p or nil, v0.x_s.ld,
                                v0.has_t and v0.xT_s.p or nil, v0.has_t and v0.x2T_s.p or nil, v0.has_t and v0.xT_s.ld or 0, 0))
    end
    -- forward: dual GEMM + noise / ReLU / operand packing in the epilogue
    for li, v in ipairs(self.vb) do
        local nxt = self.vb[li + 1]
        local fa = ffi.new('vbnn_fwd_args')
        fa.w, fa.w2, fa.x, fa.x2, fa.ld_w, fa.ld_x = v.mu_s.p, v.var_s.p, v.x_in, v.x2_s and v.x2_s.p or nil, v.mu_s.ld, v.ld_in
        fa.N, fa.I, fa.O, fa.bias = N, v.I, v.O, f32(v.bias)
        fa.seed, fa.layer, fa.draw, fa.row0 = self.seed, v.layer_id, self.draw_dev and 0 or self.draw, row0
        fa.draw_dev = self.draw_dev
        fa.r, fa.ld_r, fa.r_packed, fa.relu = v.r, v.O, 1, 1
        fa.h = nxt and nxt.x_s.p or self.h_s.p
        fa.h2 = (nxt and nxt.x2_s) and nxt.x2_s.p or nil
        fa.ld_h = nxt and nxt.x_s.ld or self.h_s.ld
        if nxt and nxt.has_t then fa.hT, fa.h2T, fa.ld_hT = nxt.xT_s.p, nxt.x2T_s.p, nxt.xT_s.ld end
        if not nxt and self.n_head_slots > 0 then
            fa.head_w3, fa.head_ld_w, fa.head_C, fa.head_slots = self.w3_s.p, self.w3_s.ld, self.n_classes, ffi.cast('float*', self.head_slots)
        end
        check(C.vbnn_forward(vb.ctx, self.dtype, fa))
    end
    -- final Linear + LogSoftMax + ClassNLL (mlp.lua:29-32), forward and backward
    local vl, H = self.vb[#self.vb], self.sizes[#self.sizes]
    local ha = ffi.new('vbnn_head_args')
    ha.h, ha.ld_h, ha.w3, ha.ld_w, ha.bias = self.h_s.p, self.h_s.ld, self.w3_s.p, self.w3_s.ld, f32(self.bias3)
    ha.target = ffi.cast('const int32_t*', targets)
    ha.N, ha.H, ha.C, ha.rows_per_draw, ha.inv_n, ha.accumulate = N, H, self.n_classes, 0, inv_n, accumulate
    ha.logits, ha.out, ha.g_logits = f32(self.logits), f32(self.out), f32(self.g_logits)
    ha.loss_sum_dev, ha.correct_dev = ffi.cast('double*', self.acc), ffi.cast('int32_t*', self.corr)
    ha.gradWeight, ha.gradBias, ha.gradBias_prev = self.gradWeight3, self.gradBias3, vl.gradBias
    ha.relu_mask, ha.r_prev_packed, ha.r_prev, ha.ld_r_prev = 1, 1, vl.r, vl.O
    ha.g_prev, ha.gv_prev, ha.ld_gp = vl.g_s.p, vl.gv_s.p, vl.g_s.ld
    if vl.has_t then ha.gT_prev, ha.gvT_prev, ha.ld_gpT = vl.gT_s.p, vl.gvT_s.p, vl.gT_s.ld end
    if self.n_head_slots > 0 then ha.logit_slots, ha.n_slots = ffi.cast('const float*', self.head_slots), self.n_head_slots end
    check(C.vbnn_head_forward_backward(vb.ctx, self.dtype, ha))
    -- backward. The argument blocks of layer li (no library call in these two):
    local function dw_block(li)
        local v = self.vb[li]
        local d = ffi.new('vbnn_dw_args')
        if v.has_t then d.xT, d.x2T, d.gT, d.gvT, d.ld_n = v.xT_s.p, v.x2T_s.p, v.gT_s.p, v.gvT_s.p, v.gT_s.ld end
        d.N, d.I, d.O, d.scale, d.accumulate = N, v.I, v.O, 1, accumulate
        d.seed, d.layer, d.draw, d.lvars = self.seed, v.layer_id, self.draw, f32(v.lvars)
        d.grad_mu, d.grad_lv, d.means, d.stats = v.grad_mu, v.grad_lv, f32(v.means), ffi.cast('double*', v.stats)
        -- the KL gradient: exact, from the fp32 parameters in the update sweep (kl_in_update: the default where the epilogue would
        -- read the bf16 shadows -- (bf16(s2) / var_hat - 1) cancels; VBLinear.lua:96-97 uses the fp32 vars) or fused here (A/B)
        d.B, d.S, d.kl_scale = self.B, self.S, self.kl_in_update and 0 or 1 / self.world
        d.gradBias = v.bias_from_dw and v.gradBias or nil
        d.x, d.x2, d.g, d.gv, d.ld_x, d.ld_g = v.x_in, v.x2_s and v.x2_s.p or nil, v.g_s.p, v.gv_s.p, v.ld_in, v.g_s.ld
        if self.dtype == C.VBNN_BF16 then d.mu_s, d.var_s, d.ld_w = v.mu_s.p, v.var_s.p, v.mu_s.ld end   -- KL terms from the shadows
        return d
    end
    local function dx_block(li)
        local v, p = self.vb[li], self.vb[li - 1]
        local xa = ffi.new('vbnn_dx_args')
        if v.use_muT then xa.wT, xa.w2T = v.muT_s.p, v.varT_s.p end
        xa.ld_wT = v.muT_s.ld
        xa.g, xa.gv, xa.ld_g, xa.N, xa.I, xa.O = v.g_s.p, v.gv_s.p, v.g_s.ld, N, v.I, v.O
        xa.x, xa.ld_x, xa.relu_mask = v.x_s.p, v.x_s.ld, 1
        xa.r_prev, xa.ld_r_prev, xa.r_prev_packed = p.r, p.O, 1
        xa.g_prev, xa.gv_prev, xa.ld_gp = p.g_s.p, p.gv_s.p, p.g_s.ld
        if p.has_t then xa.gT_prev, xa.gvT_prev, xa.ld_gpT = p.gT_s.p, p.gvT_s.p, p.gT_s.ld end
        xa.w, xa.w2, xa.ld_w = v.mu_s.p, v.var_s.p, v.mu_s.ld
        return xa
    end
    if self.direct then
        -- fp32: accGradParameters and updateGradInput of a layer are independent and go out as ONE launch where the library
        -- can carry both (vbnn_backward_pair); each tile bitwise what its own launch computes
        for li = #self.vb, 1, -1 do
            local v = self.vb[li]
            local dd = dw_block(li)
            if li > 1 then
                check(C.vbnn_backward_pair(vb.ctx, self.dtype, dx_block(li), dd))
            else
                check(C.vbnn_acc_grad_parameters(vb.ctx, self.dtype, dd))
            end
            if li < #self.vb and not v.bias_from_dw then
                check(C.vbnn_acc_grad_bias(vb.ctx, self.dtype, v.g_s.p, v.g_s.ld, N, v.O, 1, accumulate, v.gradBias))
            end
        end
    elseif self.chain then
        -- updateGradInput and accGradParameters of a layer as ONE chained launch where both run on the two-pass 256 x 256 kernel
        -- (vbnn_backward_chain); the first layer's accGradParameters is a launch of its own, last
        local order = self.chain == 'dw' and 1 or 0               -- VBNN_CHAIN_DW_FIRST / VBNN_CHAIN_DX_FIRST
        for li = #self.vb, 2, -1 do
            local v = self.vb[li]
            check(C.vbnn_backward_chain(vb.ctx, self.dtype, dx_block(li), dw_block(li), order))
            if li < #self.vb and not v.bias_from_dw then
                check(C.vbnn_acc_grad_bias(vb.ctx, self.dtype, v.g_s.p, v.g_s.ld, N, v.O, 1, accumulate, v.gradBias))
            end
        end
        local v = self.vb[1]
        check(C.vbnn_acc_grad_parameters(vb.ctx, self.dtype, dw_block(1)))
        if 1 < #self.vb and not v.bias_from_dw then
            check(C.vbnn_acc_grad_bias(vb.ctx, self.dtype, v.g_s.p, v.g_s.ld, N, v.O, 1, accumulate, v.gradBias))
        end
    elseif self.dx_first then
        for li = #self.vb, 2, -1 do
            check(C.vbnn_grad_input(vb.ctx, self.dtype, dx_block(li)))
        end
        for li = 1, #self.vb do
            local v = self.vb[li]
            check(C.vbnn_acc_grad_parameters(vb.ctx, self.dtype, dw_block(li)))
            if li < #self.vb and not v.bias_from_dw then
                check(C.vbnn_acc_grad_bias(vb.ctx, self.dtype, v.g_s.p, v.g_s.ld, N, v.O, 1, accumulate, v.gradBias))
            end
        end
    else
        -- last VB layer first: accGradParameters (+ its bucket's all-reduce), then updateGradInput
        for li = #self.vb, 1, -1 do
            local v = self.vb[li]
            local dd = dw_block(li)
            local msg_off = v.bucket_off
            local early = self.comm and v.O * v.I >= 2 ^ 22 and v.early_ok
            if early then
                -- two launches (vbnn_dw_args.part): the sigma^2 GEMM and d/dlvars first, whose exchange then starts while the
                -- mu GEMM still runs (d/dlvars is the first block of the layer's bucket)
                dd.part = 2
                check(C.vbnn_acc_grad_parameters(vb.ctx, self.dtype, dd))
                if self.sharded then self:_scatter(li, true, false, false)
                else check(C.vbnn_allreduce_grads(self.comm, f32(self.grads) + v.bucket_off, v.O * v.I)) end
                dd.part = 1
                msg_off = v.bucket_off + v.O * v.I
            end
            check(C.vbnn_acc_grad_parameters(vb.ctx, self.dtype, dd))
            if li < #self.vb and not v.bias_from_dw then
                check(C.vbnn_acc_grad_bias(vb.ctx, self.dtype, v.g_s.p, v.g_s.ld, N, v.O, 1, accumulate, v.gradBias))
            end
            if self.comm and self.sharded then
                self:_scatter(li, not early, true, true)
            elseif self.comm then                                 -- the final Linear's gradients ride in the last layer's message
                local n = ((li == #self.vb) and self.n_grads or (v.bucket_off + v.bucket_n)) - msg_off
                check(C.vbnn_allreduce_grads(self.comm, f32(self.grads) + msg_off, n))
            end
            if li > 1 then
                check(C.vbnn_grad_input(vb.ctx, self.dtype, dx_block(li)))
            end
        end
    end
    self.first = false
end

function FusedMLP:finish()                                        -- end of the minibatch: gradients complete on the stream
    if self.comm then check(C.vbnn_comm_finish(self.comm)) end
end

-- mlp:update + VBLinear:update (mlp.lua:117-142, VBLinear.lua:124-166) in one call, which also leaves the operand
-- shadows and prior statistics of the next minibatch; `log` (a FloatTensor-free double[14 * layers] on the device)
function FusedMLP:update(opt, log14)
    self:finish()
    self.version = (self.version or 0) + 1                          -- a pruned view (:prune) is a snapshot of one version
    if self.sharded then return self:_update_sharded(opt) end
    local lr = opt.state.learningRate
    local H = self.sizes[#self.sizes]
    check(C.vbnn_sgd_step(vb.ctx, f32(self.weight3), self.gradWeight3, self.n_classes * H, lr))
    check(C.vbnn_sgd_step(vb.ctx, f32(self.bias3), self.gradBias3, self.n_classes, lr))
    local n = #self.vb
    local d = ffi.new('vbnn_update_desc[?]', n)
    for k, v in ipairs(self.vb) do
        v.t = v.t + 1
        local e = d[k - 1]
        e.means, e.lvars, e.O, e.I = f32(v.means), f32(v.lvars), v.O, v.I
        e.mu_s, e.var_s, e.ld_w = v.mu_s.p, v.var_s.p, v.mu_s.ld
        e.muT_s, e.varT_s = v.use_muT and v.muT_s.p or nil, v.use_muT and v.varT_s.p or nil
        e.ld_wT = v.muT_s and v.muT_s.ld or 0
        e.stats, e.grad_mu, e.grad_lv = ffi.cast('double*', v.stats), v.grad_mu, v.grad_lv
        e.m_mu, e.v_mu, e.m_lv, e.v_lv = f32(v.m_mu), f32(v.v_mu), f32(v.m_lv), f32(v.v_lv)
        for key, st in pairs({ mu = opt.meanState, lv = opt.varState }) do
            e[key].lr, e[key].beta1, e[key].beta2 = st.learningRate, st.beta1 or 0.9, st.beta2 or 0.999
            e[key].eps, e[key].lambda, e[key].t = st.epsilon or 1e-8, st.lambda or 1, v.t
        end
        e.bias, e.grad_bias, e.lr_bias, e.B = f32(v.bias), v.gradBias, lr, self.B
        e.log14 = log14 and (ffi.cast('double*', log14) + 14 * (k - 1)) or nil
        e.kl_add = self.kl_in_update and 1 or 0
    end
    local w3 = ffi.new('vbnn_pack_desc[1]')
    w3[0].src, w3[0].rows, w3[0].cols, w3[0].ld_src = f32(self.weight3), self.n_classes, H, H
    w3[0].dst, w3[0].ld_dst, w3[0].dstT, w3[0].ld_dstT = self.w3_s.p, self.w3_s.ld, nil, 0
    if self.held then check(C.vbnn_update_masked(vb.ctx, self.dtype, n, d, self.held, w3))    -- the frozen weights keep every bit
    else check(C.vbnn_update(vb.ctx, self.dtype, n, d, w3)) end
end

-- mlp:calc_lc (mlp.lua:109-115): sum over the VB layers of VBLinear:calc_lc (VBLinear.lua:99-103), fresh statistics
function FusedMLP:calc_lc(opt)
    local lc, box, dev = 0, ffi.new('double[1]'), vb.alloc(8)
    for li, v in ipairs(self.vb) do
        if self.held then                                           -- the KL of the network that exists: the kept weights' sum
            check(C.vbnn_calc_lc_masked(vb.ctx, f32(v.means), f32(v.lvars), self.held[li - 1], ffi.cast('double*', v.stats),
                                        (opt or self.opt).B, nil, ffi.cast('double*', dev), v.O * v.I))
        else
            check(C.vbnn_calc_lc(vb.ctx, f32(v.means), f32(v.lvars), nil, nil, ffi.cast('double*', v.stats), (opt or self.opt).B, nil,
                                 ffi.cast('double*', dev), v.O * v.I))
        end
        check(C.vbnn_buf_download(vb.ctx, box, dev, 8))
        lc = lc + box[0]
    end
    return lc
end

-- error (mean NLL over the GLOBAL batch, this rank's share) and hit count of the last run(s); synchronises
function FusedMLP:loss_and_accuracy()
    self:finish()
    local a, c = ffi.new('double[2]'), ffi.new('int32_t[1]')
    check(C.vbnn_buf_download(vb.ctx, a, self.acc, 16))
    check(C.vbnn_buf_download(vb.ctx, c, self.corr, 4))
    return a[0], c[0]
end

-- structured pruning (the group form of mainviz.lua:20-21; engine.py:FusedMLP.prune_units, tools/c_host.c:fm_prune_units): every
-- hidden unit with ||mu_o|| / ||sigma_o|| < tau. Exactly one of `fraction` (0 .. 1: tau = the exact k-th smallest unit key,
-- k = floor(fraction units); 1 = tau = +inf) and `threshold` (tau itself); scope 'global' (one tau over the units of all VB layers,
-- the default) or 'layer'; `multiple` (default 1): every layer's kept count is rounded up to a multiple of it (256: widths the tiled
-- GEMM kernels take); a layer never loses its last unit. Returns a table: tau[li], keep[li] (device, uint32, ascending),
-- hidden[li] (the kept counts), layers[li] = { n_units, n_pruned, fraction_pruned } and the same three as totals, n_weights,
-- n_weights_before. :compact(result) builds the smaller network.
function FusedMLP:prune_units(fraction, threshold, scope, multiple)
    assert((fraction == nil) ~= (threshold == nil), 'prune_units: exactly one of fraction and threshold')
    assert(not self.held, 'prune_units: a pruning mask is held (:release_pruned first)')
    scope, multiple = scope or 'global', multiple or 1
    assert(scope == 'global' or scope == 'layer', "prune_units: scope 'global' or 'layer'")
    assert(fraction == nil or (fraction >= 0 and fraction <= 1), 'prune_units: fraction in 0 .. 1')
    assert(multiple >= 1 and multiple == math.floor(multiple), 'prune_units: multiple is an integer >= 1')
    assert(not self.sharded, 'prune_units: the fp32 parameters of a sharded engine are this rank\'s rows only')
    local n = #self.vb
    local o = { scope = scope, multiple = multiple, tau = {}, keep = {}, hidden = {}, layers = {} }
    local tau, n_keep, keys = vb.alloc(4 * n), vb.alloc(4 * n), {}
    for li, v in ipairs(self.vb) do keys[li], o.keep[li] = vb.alloc(4 * v.O), vb.alloc(4 * v.O) end
    local function descs(first, count)
        local d = ffi.new('vbnn_unit_desc[?]', count)
        for j = 0, count - 1 do
            local v, e = self.vb[first + j], d[j]
            e.means, e.lvars, e.O, e.I = f32(v.means), f32(v.lvars), v.O, v.I
            e.key, e.keep = f32(keys[first + j]), ffi.cast('uint32_t*', o.keep[first + j])
            e.n_keep = ffi.cast('uint32_t*', n_keep) + (first + j - 1)
        end
        return d
    end
    check(C.vbnn_unit_snr(vb.ctx, n, descs(1, n)))
    local select = fraction ~= nil and fraction < 1                -- else the threshold is a host value
    local groups = (scope == 'global') and { { 1, n } } or {}
    if scope == 'layer' then for li = 1, n do groups[li] = { li, 1 } end end
    for _, g in ipairs(groups) do
        if select then                                             -- the threshold stays on the device, behind the select
            local units = 0
            for li = g[1], g[1] + g[2] - 1 do units = units + self.vb[li].O end
            local k = math.min(math.floor(fraction * units), units - 1)
            check(C.vbnn_unit_select(vb.ctx, g[2], descs(g[1], g[2]), k, f32(tau) + (g[1] - 1)))
        end
    end
    local tau_host = threshold or math.huge
    check(C.vbnn_unit_index(vb.ctx, n, descs(1, n), select and f32(tau) or nil, tau_host, multiple))
    local nh, th = ffi.new('uint32_t[?]', n), ffi.new('float[?]', n)
    check(C.vbnn_buf_download(vb.ctx, nh, n_keep, 4 * n))
    if select then check(C.vbnn_buf_download(vb.ctx, th, tau, 4 * n)) end
    local function weights(sizes)
        local w = sizes[#sizes] * self.n_classes
        for k = 1, #sizes - 1 do w = w + sizes[k] * sizes[k + 1] end
        return w
    end
    local sizes, units, kept = { self.sizes[1] }, 0, 0
    for li, v in ipairs(self.vb) do
        local nk = tonumber(nh[li - 1])
        o.tau[li] = select and th[li - 1] or tau_host
        o.hidden[li], sizes[li + 1] = nk, nk
        o.layers[li] = { n_units = v.O, n_pruned = v.O - nk, fraction_pruned = (v.O - nk) / v.O }
        units, kept = units + v.O, kept + nk
    end
    o.n_units, o.n_pruned, o.fraction_pruned = units, units - kept, (units - kept) / units
    o.n_weights, o.n_weights_before = weights(sizes), weights(self.sizes)
    o.owner, o.version, o.units = self, self.version or 0, true
    return o
end

-- The network a :prune_units result leaves (engine.py:FusedMLP.compact, tools/c_host.c:fm_compact): a new FusedMLP with
-- hidden = result.hidden (one process), its parameters gathered on the device -- a layer's rows by its own kept list, its columns
-- by the previous layer's, the final weight by the last list; the final bias copied (a plain gather), the draw counter advanced to this one's -- and
-- prepared. Fresh optimiser state; the removed units' constant activations are dropped. `overrides`: options that differ.
function FusedMLP:compact(result, overrides)
    assert(result and result.units and result.owner == self, 'compact: a result of this :prune_units')
    assert(result.version == (self.version or 0), 'compact: the parameters changed since this result was taken')
    local opt = {}
    for k, v in pairs(self.opt) do opt[k] = v end
    opt.world, opt.rank, opt.comm_id, opt.exchange_mode = nil, nil, nil, nil
    for k, v in pairs(overrides or {}) do opt[k] = v end
    opt.hidden = result.hidden
    local new = FusedMLP.new(opt)
    local ga = ffi.new('vbnn_unit_gather_args')
    local cols = nil
    for li, v in ipairs(self.vb) do
        local w = new.vb[li]
        ga.means, ga.lvars, ga.bias, ga.O, ga.I = f32(v.means), f32(v.lvars), f32(v.bias), v.O, v.I
        ga.rows, ga.n_rows, ga.cols, ga.n_cols = ffi.cast('uint32_t*', result.keep[li]), w.O, cols, w.I
        ga.dst_means, ga.dst_lvars, ga.dst_bias = f32(w.means), f32(w.lvars), f32(w.bias)
        check(C.vbnn_unit_gather(vb.ctx, ga))
        cols = ffi.cast('uint32_t*', result.keep[li])
    end
    ga.means, ga.lvars, ga.bias, ga.O, ga.I = f32(self.weight3), nil, nil, self.n_classes, self.sizes[#self.sizes]
    ga.rows, ga.n_rows, ga.cols, ga.n_cols = nil, self.n_classes, cols, new.sizes[#new.sizes]
    ga.dst_means, ga.dst_lvars, ga.dst_bias = f32(new.weight3), nil, nil
    check(C.vbnn_unit_gather(vb.ctx, ga))
    ga.means, ga.O, ga.I, ga.n_rows, ga.cols, ga.n_cols, ga.dst_means = f32(self.bias3), 1, self.n_classes, 1, nil, self.n_classes, f32(new.bias3)
    check(C.vbnn_unit_gather(vb.ctx, ga))
    new.draw = self.draw
    if new.draw_dev then check(C.vbnn_sample(vb.ctx, new.draw_dev, self.draw)) end   -- its device counter starts at zero
    new:prepare()
    return new
end

-- signal-to-noise pruning (mainviz.lua:20-27; engine.py:FusedMLP.prune, tools/c_host.c:fm_prune): every weight with
-- |mu| / sigma < tau. Exactly one of `fraction` (0 .. 1: tau = the exact k-th smallest key, k = floor(fraction W); 1 = everything,
-- tau = +inf) and `threshold` (tau itself; the reference's 0.005); scope 'global' (one tau over all VB layers, the default) or
-- 'layer' (the fraction per layer). Returns a table: tau[li], layers[li] = { n_pruned, W, fraction_pruned, mean_var,
-- mean_pruned_var }, the same five as totals (the numbers mainviz.lua:22-27 prints), and the pruned operand shadows mu_p[li] /
-- var_p[li] that predict() reads once the table is handed to use_pruned.
function FusedMLP:prune(fraction, threshold, scope)
    assert((fraction == nil) ~= (threshold == nil), 'prune: exactly one of fraction and threshold')
    scope = scope or 'global'
    assert(scope == 'global' or scope == 'layer', "prune: scope 'global' or 'layer'")
    assert(fraction == nil or (fraction >= 0 and fraction <= 1), 'prune: fraction in 0 .. 1')
    local n = #self.vb
    local o = { scope = scope, tau = {}, layers = {}, mu_p = {}, var_p = {} }
    local stats, tau = vb.alloc(32 * n), vb.alloc(4 * n)
    local function descs(first, count)
        local d = ffi.new('vbnn_prune_desc[?]', count)
        for j = 0, count - 1 do
            local v, e = self.vb[first + j], d[j]
            e.means, e.lvars, e.O, e.I = f32(v.means), f32(v.lvars), v.O, v.I
            e.mu_p, e.var_p, e.ld_w = o.mu_p[first + j].p, o.var_p[first + j].p, o.mu_p[first + j].ld
            e.stats = ffi.cast('double*', stats) + 4 * (first + j - 1)
            e.mask = nil
        end
        return d
    end
    for li, v in ipairs(self.vb) do o.mu_p[li], o.var_p[li] = packed(v.O, v.I, self.esize), packed(v.O, v.I, self.esize) end
    local nbytes = ffi.new('size_t[1]')
    check(C.vbnn_prune_workspace_bytes(n, descs(1, n), nbytes))
    local ws = vb.alloc(tonumber(nbytes[0]))
    local groups = (scope == 'global') and { { 1, n } } or {}
    if scope == 'layer' then for li = 1, n do groups[li] = { li, 1 } end end
    local selected = {}
    for _, g in ipairs(groups) do
        local d, Wg = descs(g[1], g[2]), 0
        for li = g[1], g[1] + g[2] - 1 do Wg = Wg + self.vb[li].O * self.vb[li].I end
        local k = fraction and math.floor(fraction * Wg) or Wg
        local tau_g = nil
        if k < Wg then                                             -- the threshold stays on the device, behind the select
            tau_g = f32(tau) + (g[1] - 1)
            check(C.vbnn_prune_select(vb.ctx, g[2], d, k, tau_g, ws, nbytes[0]))
        end
        check(C.vbnn_prune_pack(vb.ctx, self.dtype, g[2], d, tau_g, threshold or math.huge))
        for li = g[1], g[1] + g[2] - 1 do selected[li] = tau_g and g[1] or false end
    end
    local sh, th = ffi.new('double[?]', 4 * n), ffi.new('float[?]', n)
    check(C.vbnn_buf_download(vb.ctx, sh, stats, 32 * n))
    check(C.vbnn_buf_download(vb.ctx, th, tau, 4 * n))
    local function summary(np, sp, sa, W)
        return { n_pruned = np, W = W, fraction_pruned = np / W, mean_var = sa / W, mean_pruned_var = sp / np }
    end
    local tot = { 0, 0, 0, 0 }
    for li = 1, n do
        o.tau[li] = selected[li] and th[selected[li] - 1] or (threshold or math.huge)
        o.layers[li] = summary(sh[4 * li - 4], sh[4 * li - 3], sh[4 * li - 2], sh[4 * li - 1])
        for j = 1, 4 do tot[j] = tot[j] + sh[4 * li - 5 + j] end
    end
    local t = summary(tot[1], tot[2], tot[3], tot[4])
    o.n_pruned, o.W, o.fraction_pruned, o.mean_var, o.mean_pruned_var = t.n_pruned, t.W, t.fraction_pruned, t.mean_var, t.mean_pruned_var
    o.owner, o.version = self, self.version or 0
    return o
end

-- predict() reads the pruned operands of `result` (a table from :prune) from now on; nil: the unpruned shadows again. Nothing
-- else looks at the view. A view is a snapshot: prune again after update() (self.version counts the updates).
function FusedMLP:use_pruned(result)
    assert(result == nil or result.owner == self, 'use_pruned: a result of this :prune, or nil')
    assert(result == nil or result.version == (self.version or 0), 'use_pruned: the parameters changed since this result was taken')
    self.pruned_view = result
end

-- Training the network a pruning leaves (engine.py:FusedMLP.hold_pruned, tools/c_host.c:fm_hold_pruned): the weights `result` (a
-- table from :prune, of the current version) prunes are out of the network AND frozen from now on -- :prepare / :update / :calc_lc
-- take the masked entry points (+0 in the shadows, parameters and Adam moments untouched, the kept weights' prior statistics); :run
-- is unchanged. The byte masks come from one more vbnn_prune_pack per layer at the result's own tau. Returns the held counts per
-- layer. One pruning at a time here: the library has no call that ORs two masks, so an iterative schedule (hold, train, prune
-- again, hold the union) is the Python engine's; :release_pruned first. Not with the sharded update; a layer must keep a weight.
-- :prune_units / :compact / :compress read the fp32 parameters, which still hold the frozen values: release before them.
function FusedMLP:hold_pruned(result)
    assert(result and result.owner == self and not result.sparse, 'hold_pruned: a (dense) result of this :prune')
    assert(result.version == (self.version or 0), 'hold_pruned: the parameters changed since this result was taken')
    assert(not self.sharded, 'hold_pruned: not with the sharded update')
    assert(not self.held, 'hold_pruned: a mask is held already (:release_pruned first)')
    local n = #self.vb
    -- (bufs owns the masks: vb.alloc's cdata frees its buffer when collected, and neither a cast nor the pointer array keeps it alive)
    local held, counts, bufs = ffi.new('const uint8_t*[?]', n), {}, {}
    local stats = vb.alloc(32)
    for li, v in ipairs(self.vb) do
        assert(result.layers[li].n_pruned < v.O * v.I, 'hold_pruned: a layer would be left without a kept weight')
        local mask = vb.alloc(v.O * v.I)
        local d = ffi.new('vbnn_prune_desc[1]')
        d[0].means, d[0].lvars, d[0].O, d[0].I = f32(v.means), f32(v.lvars), v.O, v.I
        d[0].mu_p, d[0].var_p, d[0].ld_w = result.mu_p[li].p, result.var_p[li].p, result.mu_p[li].ld   -- the same sweep: the same bits
        d[0].stats, d[0].mask = ffi.cast('double*', stats), ffi.cast('uint8_t*', mask)
        check(C.vbnn_prune_pack(vb.ctx, self.dtype, 1, d, nil, result.tau[li]))
        held[li - 1], counts[li], bufs[li] = ffi.cast('const uint8_t*', mask), result.layers[li].n_pruned, mask
    end
    self.held, self.held_counts, self.held_bufs = held, counts, bufs
    self.version = (self.version or 0) + 1                          -- shadows and statistics change: earlier results are void
    self:prepare()
    return counts
end

-- drops the held mask and runs the ordinary :prepare: the frozen weights are back with the values they were held with
function FusedMLP:release_pruned()
    self.held, self.held_counts, self.held_bufs = nil, nil, nil
    self.version = (self.version or 0) + 1
    self:prepare()
end

-- The compressed form of a :prune result (engine.py:FusedMLP._compress, tools/c_host.c:fm_compress): the kept weights only, CSR per
-- layer over output rows (include/vbnn_hip.h: vbnn_sparse_desc), built on the device at the result's own tau; the entry count is
-- W - n_pruned, known from the result. Returns a result :use_pruned takes like any other; under it predict() multiplies by the
-- entries directly (:_predict_forward_sparse). It owns no dense shadows.
function FusedMLP:compress(result)
    assert(result and result.owner == self, 'compress: a result of this :prune')
    assert(not self.held, 'compress: a pruning mask is held (:release_pruned first)')
    assert(result.version == (self.version or 0), 'compress: the parameters changed since this result was taken')
    if result.sparse then return result end
    local n = #self.vb
    local o = { scope = result.scope, tau = result.tau, layers = result.layers, sparse = true, owner = self, version = result.version,
                n_pruned = result.n_pruned, W = result.W, fraction_pruned = result.fraction_pruned, mean_var = result.mean_var,
                mean_pruned_var = result.mean_pruned_var, row_ptr = {}, cols = {}, mu_v = {}, var_v = {}, nnz = {}, idx_bytes = {},
                nbytes = 0, dense_nbytes = 0 }
    local nnz_dev = vb.alloc(4 * n)
    for li, v in ipairs(self.vb) do
        local nnz = result.layers[li].W - result.layers[li].n_pruned
        local ib, cap = (v.I <= 65536) and 2 or 4, math.max(nnz, 1)
        o.nnz[li], o.idx_bytes[li] = nnz, ib
        o.row_ptr[li], o.cols[li] = vb.alloc(4 * (v.O + 1)), vb.alloc(ib * cap)
        o.mu_v[li], o.var_v[li] = vb.alloc(self.esize * cap), vb.alloc(self.esize * cap)
        o.nbytes = o.nbytes + 4 * (v.O + 1) + (ib + 2 * self.esize) * cap
        o.dense_nbytes = o.dense_nbytes + 2 * v.O * vb.pad_ld(v.I) * self.esize
        local d, sd = ffi.new('vbnn_prune_desc[1]'), ffi.new('vbnn_sparse_desc[1]')
        d[0].means, d[0].lvars, d[0].O, d[0].I = f32(v.means), f32(v.lvars), v.O, v.I
        sd[0].row_ptr, sd[0].cols, sd[0].mu_v, sd[0].var_v = ffi.cast('uint32_t*', o.row_ptr[li]), o.cols[li], o.mu_v[li], o.var_v[li]
        sd[0].O, sd[0].I, sd[0].nnz_cap, sd[0].idx_bytes = v.O, v.I, nnz, ib
        sd[0].nnz_dev = ffi.cast('uint32_t*', nnz_dev) + (li - 1)
        check(C.vbnn_prune_compress(vb.ctx, self.dtype, 1, d, sd, nil, result.tau[li]))
    end
    local got = ffi.new('uint32_t[?]', n)
    check(C.vbnn_buf_download(vb.ctx, got, nnz_dev, 4 * n))
    for li = 1, n do assert(got[li - 1] == o.nnz[li], 'compress: the device kept another number of weights than the pruning counted') end
    return o
end

-- predict's forwards under a compressed view: the input packed with its transpose, then every VB layer on its entries -- K-major
-- activations from layer to layer (xT[li]: layer li's input), the last layer writes the row-major h the head reads
function FusedMLP:_predict_forward_sparse(in_x, x, ld, N, rpd, draw, row0, pack)
    local pv = self.pruned_view
    if not pv.xT or pv.xT_rows ~= in_x[1].rows then
        pv.xT, pv.xT_rows = {}, in_x[1].rows
        for li = 1, #self.vb do pv.xT[li] = packed(self.sizes[li], in_x[1].rows, self.esize) end
    end
    if pack then
        check(C.vbnn_pack_input(vb.ctx, self.dtype, x, ld, N, self.sizes[1], in_x[1].p, nil, in_x[1].ld, pv.xT[1].p, nil, pv.xT[1].ld, rpd))
    end
    for li, v in ipairs(self.vb) do
        local sa = ffi.new('vbnn_sparse_fwd_args')
        sa.row_ptr, sa.cols, sa.mu_v, sa.var_v = ffi.cast('const uint32_t*', pv.row_ptr[li]), pv.cols[li], pv.mu_v[li], pv.var_v[li]
        sa.idx_bytes, sa.xT, sa.x2T, sa.ld_xT = pv.idx_bytes[li], pv.xT[li].p, nil, pv.xT[li].ld
        sa.N, sa.I, sa.O, sa.bias = N, v.I, v.O, f32(v.bias)
        sa.seed, sa.layer, sa.draw, sa.row0 = self.seed, v.layer_id, draw, row0
        sa.relu, sa.rows_per_draw = 1, rpd
        if li == #self.vb then
            sa.h, sa.ld_h = in_x[li + 1].p, in_x[li + 1].ld
        else
            sa.hT, sa.ld_hT = pv.xT[li + 1].p, pv.xT[li + 1].ld
        end
        check(C.vbnn_forward_sparse(vb.ctx, self.dtype, sa))
    end
end

-- the posterior predictive (engine.py:FusedMLP.predict, tools/c_host.c:fm_predict): mlp:test's S draws averaged as probabilities
-- (mlp.lua:86-107, main.lua:55-74, visualize.lua:66-100), forward-only on buffers of its own (in_x[li]: layer li's input,
-- in_x[#vb + 1] the head's; r: a throwaway noise factor for the one-draw bf16 forwards). Consumes draws draw + 1 .. draw + S, as
-- mlp:test does. Returns a table of device buffers -- probs, log_probs (R x C floats), entropy, expected_entropy, mutual_info
-- (R floats), pred (R int32) -- and, with targets, nll / accuracy of the average and mean_draw_nll / mean_draw_accuracy (the two
-- numbers mlp:test returns), accuracies in percent. opt: predict_rows (32768), predict_stacked ('auto' / true / false).
function FusedMLP:predict(inputs, ld, targets, R, S, opt)
    opt = opt or {}
    assert(not self.pruned_view or self.pruned_view.version == (self.version or 0), 'predict: the pruned view is of older parameters')
    local nc, cap = self.n_classes, opt.predict_rows or 32768
    local widest, omax = 0, 0
    for _, v in ipairs(self.vb) do widest, omax = math.max(widest, v.I * v.O), math.max(omax, v.O) end
    local stacked
    if S == 1 then
        stacked = true
    elseif opt.predict_stacked ~= nil and opt.predict_stacked ~= 'auto' then
        stacked = opt.predict_stacked
    else
        stacked = math.min(R, cap) * widest < 2 ^ 32              -- one draw's widest forward small: S launches become one
    end
    local Rc = math.max(1, math.min(R, stacked and math.floor(cap / S) or cap))
    local rows = stacked and S * Rc or Rc
    local sq = self.dtype == C.VBNN_BF16                           -- (fp32: the forward forms x.x from x itself)
    local in_x, in_x2 = {}, {}
    for li = 1, #self.vb + 1 do
        in_x[li] = packed(rows, self.sizes[li], self.esize)
        if sq and li <= #self.vb then in_x2[li] = packed(rows, self.sizes[li], self.esize) end
    end
    local r = sq and packed(rows, omax, self.esize) or nil
    local chunks = math.floor((R + Rc - 1) / Rc)
    local o = { R = R, S = S, stacked = stacked, chunks = chunks }
    o.probs, o.log_probs = vb.alloc(R * nc * 4), vb.alloc(R * nc * 4)
    o.entropy, o.expected_entropy, o.mutual_info, o.pred = vb.alloc(R * 4), vb.alloc(R * 4), vb.alloc(R * 4), vb.alloc(R * 4)
    local totals = vb.alloc(chunks * 32)
    local state = (not stacked) and vb.alloc(Rc * (nc + 3) * 4) or nil
    local d0, row0 = self.draw + 1, self.rank * R                 -- the first draw's counter (sample() then run())
    local pa = ffi.new('vbnn_predict_args')
    pa.w3, pa.ld_w, pa.bias, pa.H, pa.C, pa.S = self.w3_s.p, self.w3_s.ld, f32(self.bias3), self.sizes[#self.sizes], nc, S
    pa.form = stacked and C.VBNN_PREDICT_STACKED or C.VBNN_PREDICT_ACCUMULATE
    pa.state = state and f32(state) or nil
    for k = 0, chunks - 1 do
        local c0 = k * Rc
        local n = math.min(Rc, R - c0)
        local xc = f32(inputs) + c0 * ld
        pa.h, pa.ld_h, pa.R = in_x[#self.vb + 1].p, in_x[#self.vb + 1].ld, n
        pa.target = targets and (ffi.cast('const int32_t*', targets) + c0) or nil
        pa.totals = targets and (ffi.cast('double*', totals) + 4 * k) or nil
        pa.probs, pa.log_probs = f32(o.probs) + c0 * nc, f32(o.log_probs) + c0 * nc
        pa.entropy, pa.expected_entropy, pa.mutual_info = f32(o.entropy) + c0, f32(o.expected_entropy) + c0, f32(o.mutual_info) + c0
        pa.pred = ffi.cast('int32_t*', o.pred) + c0
        if stacked then                                            -- every draw in one pass: the chunk stacked S times as rows
            self:_predict_forward(in_x, in_x2, r, xc, ld, S * n, S > 1 and n or 0, d0, row0 + c0, true)
            check(C.vbnn_head_predict(vb.ctx, self.dtype, pa))
        else                                                       -- one draw per forward, the running state between the launches
            for s = 0, S - 1 do
                self:_predict_forward(in_x, in_x2, r, xc, ld, n, 0, d0 + s, row0 + c0, s == 0)
                pa.first, pa.final = (s == 0) and 1 or 0, (s == S - 1) and 1 or 0
                check(C.vbnn_head_predict(vb.ctx, self.dtype, pa))
            end
        end
    end
    self.draw = self.draw + S
    if self.draw_dev then check(C.vbnn_sample(vb.ctx, self.draw_dev, S)) end
    if targets then                                                -- the chunks' totals, added in chunk order
        local th = ffi.new('double[?]', 4 * chunks)
        check(C.vbnn_buf_download(vb.ctx, th, totals, 32 * chunks))
        local tot = { 0, 0, 0, 0 }
        for k = 0, chunks - 1 do
            for j = 1, 4 do tot[j] = tot[j] + th[4 * k + j - 1] end
        end
        o.totals = tot
        o.nll, o.accuracy = tot[1] / R, 100 * tot[2] / R
        o.mean_draw_nll, o.mean_draw_accuracy = tot[3] / (R * S), 100 * tot[4] / (R * S)
    end
    return o
end

-- predict's forwards: the input packed (stacked draws: rows_per_draw), then every VB layer; r only for one-draw forwards
function FusedMLP:_predict_forward(in_x, in_x2, r, x, ld, N, rpd, draw, row0, pack)
    if self.pruned_view and self.pruned_view.sparse then           -- the compressed view: its own forward (above :predict)
        return self:_predict_forward_sparse(in_x, x, ld, N, rpd, draw, row0, pack)
    end
    if pack then
        check(C.vbnn_pack_input(vb.ctx, self.dtype, x, ld, N, self.sizes[1], in_x[1].p, in_x2[1] and in_x2[1].p or nil, in_x[1].ld,
                                nil, nil, 0, rpd))
    end
    for li, v in ipairs(self.vb) do
        local fa = ffi.new('vbnn_fwd_args')
        local pv = self.pruned_view                                -- a pruned view (:use_pruned): ITS shadows in place of mu_s / var_s
        local mu, var = pv and pv.mu_p[li] or v.mu_s, pv and pv.var_p[li] or v.var_s
        fa.w, fa.w2, fa.x, fa.ld_w, fa.ld_x = mu.p, var.p, in_x[li].p, mu.ld, in_x[li].ld
        fa.x2 = in_x2[li] and in_x2[li].p or nil
        fa.N, fa.I, fa.O, fa.bias = N, v.I, v.O, f32(v.bias)
        fa.seed, fa.layer, fa.draw, fa.row0, fa.draw_dev = self.seed, v.layer_id, draw, row0, nil
        if rpd == 0 and r then fa.r, fa.ld_r = r.p, r.ld end
        fa.r_packed, fa.relu, fa.rows_per_draw = 1, 1, rpd
        fa.h, fa.ld_h = in_x[li + 1].p, in_x[li + 1].ld
        fa.h2 = (li < #self.vb and in_x2[li + 1]) and in_x2[li + 1].p or nil
        check(C.vbnn_forward(vb.ctx, self.dtype, fa))
    end
end

return FusedMLP
