// sampler.h -- the fused sampler step (device code; included by warehouse_amd.hip after
// step_loops.h, whose FastRun and run_steps it steps with, and observe.h, whose row writer it
// streams with): FImg, SampLds, write_image, k_sampler.
// ----------------------------------------------------------------------------- fused sampler step
// The sampler route (wh_sampler_step: device policy + step + auto-reset, then the observation rows)
// as ONE launch.  A workgroup of 2 x BT lanes owns BT envs: lanes [0, BT) run the fused rollout's
// step for one env each (exactly k_step's fast instance, one step, lane = env), and write their
// env's byte image straight from the registers and the pickup plane; then all 2 x BT lanes stream the
// group's contiguous rows [BT x NA x L] f32 from the images, as k_observe's write loop does.
// Against k_step + k_observe: no second launch, no re-read of the state, no per-env image pass.
// Measured write phase of this shape (tools/obs_write_probe.hip, Medium-8): 512 lanes and 256 envs
// per workgroup stream at the constant-store ceiling (6.45 TB/s); 256 lanes alone (the step
// launch's own shape) reach half of it, so the second half of the workgroup is what makes the rows
// fast.  Two waves per SIMD cap the step code at 256 registers per lane.
//
// Image layout (FImg): word/half-word aligned sections so the step lanes write them with b16/b32
// stores; the compile-time gather table kObsSrcF uses the same offsets.
template <int R>
struct FImg {
  static constexpr int A0 = 1, G0 = (R + 2) & ~1, P0 = G0 + 2 * R, Q0 = (P0 + 2 * R + 3) & ~3,
                       IMG = Q0 + 4 * R;
  static_assert(IMG <= 256, "image byte offsets are 8-bit gather indices");
};
template <int R, int NAM>
__constant__ ObsSrc<R, NAM> kObsSrcF =
    make_obs_src<R, NAM, FImg<R>::A0, FImg<R>::G0, FImg<R>::P0, FImg<R>::Q0>();

template <class C, int NBUF = 1>
struct SampLds {
  static constexpr int IMG = FImg<C::R>::IMG, SRCW = ObsSrc<C::R, C::NAM>::W;
  // multi-step launches: two image buffers, step k's images written while step k-1's rows stream
  // from the other
  alignas(16) uint8_t img[NBUF][BT][IMG];
  uint32_t lim[NBUF][BT];  // n * L (floats of live rows) | fresh << 31
  uint32_t src[2][SRCW];
};

// core.py:224-260 / 371-432 for the env of this lane, from its registers after the step: the image
// k_observe builds from the packed state (n, availability, delivery targets, positions, the open
// requests in ascending pickup order with their pickup and delivery cells).
template <class C, int NBUF>
__device__ __forceinline__ void write_image(const Regs<C>& s, const Lds<C>& L, SampLds<C, NBUF>& O, int tid, int na,
                                            int buf) {
  using F = FImg<C::R>;
  uint8_t* im = O.img[buf][tid];
  uint32_t n = (s.hdr >> 16) & 0xFFu;
  n = n < (uint32_t)na ? n : (uint32_t)na;
  const bool fresh = (s.hdr >> 24) & 1u;
  constexpr uint32_t nul = (uint32_t)(C::D / 2), nul2 = nul | (nul << 8);
  im[0] = (uint8_t)n;
#pragma unroll
  for (int r = 0; r < C::R; ++r) {
    const uint32_t a = r < C::NAM ? s.ag[r] : IDLE;
    const bool live = (uint32_t)r < n;
    const bool carry = (a & 0xFF00u) != 0xFF00u;
    im[F::A0 + r] = (uint8_t)((live && !fresh && !carry) ? 1 : 0);
    const uint32_t dtg = __builtin_amdgcn_perm(a, a, 0x0C0C0301u);   // dx | dy << 8
    const uint32_t pos = __builtin_amdgcn_perm(a, a, 0x0C0C0200u);   // x | y << 8
    *reinterpret_cast<uint16_t*>(im + F::G0 + 2 * r) = (uint16_t)((live && !fresh && carry) ? dtg : nul2);
    *reinterpret_cast<uint16_t*>(im + F::P0 + 2 * r) = (uint16_t)(live ? pos : nul2);
  }
  // open requests, ascending pickup index (core.py:409-418); fewer than R open (never after a
  // reset or a step) leaves zero slots, as k_observe does
  uint32_t mlo = (uint32_t)s.am, mhi = (uint32_t)(s.am >> 32);
#pragma unroll
  for (int r = 0; r < C::R; ++r) {
    uint32_t flo, fhi;
    asm("v_ffbl_b32 %0, %1" : "=v"(flo) : "v"(mlo));   // 0xFFFFFFFF when empty
    asm("v_ffbl_b32 %0, %1" : "=v"(fhi) : "v"(mhi));
    const uint32_t j = __builtin_elementwise_min(
        __builtin_elementwise_min(flo, __builtin_elementwise_add_sat(fhi, 32u)), (uint32_t)C::P);
    const uint32_t rp = L.rtag(j).x;                        // pickup cell x | y << 16
    const uint32_t tb = L.target_byte(j, tid);              // target + 1 (row P: scratch)
    const uint32_t dc = L.dst_tb(tb);                       // x << 8 | y << 24 | 0x00FF00FF
    const uint32_t w = __builtin_amdgcn_perm(dc, rp, 0x07050200u);   // px | py << 8 | dx << 16 | dy << 24
    *reinterpret_cast<uint32_t*>(im + F::Q0 + 4 * r) = j < (uint32_t)C::P ? w : 0u;
    uint64_t m = ((uint64_t)mhi << 32) | mlo;
    m &= m - 1ull;
    mlo = (uint32_t)m;
    mhi = (uint32_t)(m >> 32);
  }
  O.lim[buf][tid] = n * (uint32_t)C::L | (fresh ? 0x80000000u : 0u);
}

// Rows of the workgroup's envs from image buffer `buf`: one contiguous [nenv x na x L] f32 region at
// `rows` (its first env's first float), float4 per lane over all 2 x BT lanes, q = tid + 2 BT i (na * L
// % 4 == 0 and 16-byte alignment: checked on the host).  (Chunks handed out from an LDS counter, so
// that the step lanes of a multi-step launch take less once they join late, measured 1.5 us slower
// on a 1-step launch and no faster on 20- and 100-step ones: profiles/r04_rows_ab.txt.)
// Every LDS read of a float4 is unconditional (a dead value reads a byte of the image, or past it,
// which LDS returns as 0 without a fault, and is then selected away): the conditional form compiled
// to one branch and one lgkmcnt(0) round trip per float, four serial LDS latencies per store.  The
// gather word of both tables is read beside lim, so a float4 costs two LDS round trips, and RU
// float4s per lane are in flight together.
template <class C, bool NTS, int NBUF>
__device__ __forceinline__ void write_rows(const SampLds<C, NBUF>& O, int buf, float* __restrict__ rows,
                                           uint32_t nenv, uint32_t qe, int tid) {
  stream_rows<2 * BT, SampLds<C, NBUF>::IMG, NTS>(O.lim[buf], O.src[0], O.src[1], &O.img[buf][0][0],
                                             reinterpret_cast<f32x4*>(rows), nenv, qe, tid);
}

// FAST: the fused rollout's steps (greedy/random policy, every env stepped, auto-reset): a.steps of
// them in one launch (wh_sampler_step: 1; wh_sampler_rollout: a rollout fragment), step k's rows
// going to obs + k * B * NA * L.  Iteration k of the launch loop: the step lanes compute step k and
// write its images into buffer k % 2 while the other lanes (and the step lanes, once done) stream
// step k-1's rows from buffer (k-1) % 2; one barrier per iteration.  So after the first step the
// simulation runs under the row stream, which is what binds (HBM writes).  State stays in registers
// across the steps, as in the fused rollout (reset slots from 8 steps on).
// Otherwise (FAST = false) wh_vector_step's single step: external actions in ascending or
// action-dict order (ORDERED), an optional env mask -- envs not stepped keep their state and still
// get their rows -- and the launch options of k_step's generic instance (episode metrics, odd agent
// counts).
template <class C, int POLICY, bool ORDERED, bool FAST, bool MULTI = false>
__global__ __launch_bounds__(2 * BT) void k_sampler(StepParams a, float* __restrict__ obs) {
  __shared__ Lds<C> L;
  __shared__ SampLds<C, MULTI ? 2 : 1> O;
  __shared__ std::conditional_t<MULTI, Slots<C>, NoSlots> RS;   // reset slots: multi-step launches
  __shared__ std::conditional_t<ORDERED, OKeys<C>, NoSlots> OK;   // dict-order move keys: ORDERED only
  const int tid = threadIdx.x;
  const bool stepper = tid < BT;
  const int64_t e0 = (int64_t)blockIdx.x * BT;
  const int64_t e = e0 + tid;
  const bool loaded = stepper && e < a.B;                              // its rows are written
  const bool stepped = loaded && (FAST || !a.mask || a.mask[e]);       // and it is stepped
  const int na = FAST ? C::NAM : a.na;
  RawEnv<C> raw;
  FastRun<C, POLICY, MULTI> run(a, e);
  // The step waves (stepper is wave-uniform: waves 0-3) issue the table loads (L2), then the state
  // planes (HBM), and write the table to LDS once it has landed, with the state still in flight --
  // all inside one uniform branch, so the waitcnt pass counts exactly (every step lane loads: a lane
  // past B re-reads env e0, which exists).  The row waves copy the gather table meanwhile.
  if (stepper) {
    const uint4 tv0 = issue_table_chunk<C>(a.tables, 0), tv1 = issue_table_chunk<C>(a.tables, 1);
    __builtin_amdgcn_sched_barrier(0);   // table loads ahead of the state loads, as in k_step
    load_env_issue<C>(raw, a.state, a.B, e0, loaded ? tid : 0, na);
    if constexpr (FAST) {
      if (loaded) run.load_actions(a, e);
    }
    commit_table_chunk<C>(L.tbl, 0, tv0);
    commit_table_chunk<C>(L.tbl, 1, tv1);
  } else {
    // all loads first, then the LDS writes: one memory latency, not one per strided iteration
    const uint32_t* srcg = &kObsSrcF<C::R, C::NAM>.w[0][0];
    constexpr int NS = 2 * SampLds<C>::SRCW, NSRC = (NS + BT - 1) / BT;
    uint32_t sv[NSRC];
#pragma unroll
    for (int i = 0; i < NSRC; ++i) sv[i] = tid - BT + i * BT < NS ? srcg[tid - BT + i * BT] : 0u;
#pragma unroll
    for (int i = 0; i < NSRC; ++i)
      if (tid - BT + i * BT < NS) (&O.src[0][0])[tid - BT + i * BT] = sv[i];
  }
  __syncthreads();
  const uint32_t nenv = (uint32_t)((a.B - e0) < BT ? (a.B - e0) : BT);
  const uint32_t qe = FAST ? (uint32_t)(C::NAM * C::L / 4) : (uint32_t)(na * C::L / 4);
  const Keys k{a.k0, a.k1};
  const uint32_t gid = (uint32_t)(a.env_offset + e);
  Regs<C> s;
  if (loaded) {
    load_env_finish<C>(s, L, raw, (uint32_t)a.W, tid);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): drain the state loads before the step (k_step)
    if (stepped) {
#pragma unroll
      for (int y = 0; y < C::D; ++y) L.occ[y][tid] = 0u;
    }
  }
  if constexpr (FAST && MULTI) {
    if (loaded) RS.rs_ep[tid] = s.epi;   // reset slots start stale (!= epi + 1)
    const int64_t step_floats = a.B * (int64_t)(C::NAM * C::L);
    const int ablate = WH_ABLATE_WORD(a);   // timing-only: 512 = no steps/images, 256 = no rows
    for (int it = 0; it <= a.steps; ++it) {   // (every wave reaches every barrier)
      if (loaded && it < a.steps && !(ablate & 512)) {
        run.step(a, s, L, &RS, k, gid, e, tid, it);
        write_image<C>(s, L, O, tid, C::NAM, it & 1);
      }
      if (it > 0 && !(ablate & 256))
        write_rows<C, false>(O, (it - 1) & 1, obs + (int64_t)(it - 1) * step_floats + e0 * (int64_t)(4 * qe), nenv, qe, tid);
      __syncthreads();
    }
    if (loaded) store_env<C>(s, L, a.state, a.B, e0, na, tid);
  } else if constexpr (FAST) {   // one step
    if (loaded) {
      run.step(a, s, L, nullptr, k, gid, e, tid, 0);
      store_env<C>(s, L, a.state, a.B, e0, na, tid);
      write_image<C>(s, L, O, tid, C::NAM, 0);
    }
    __syncthreads();
    write_rows<C, rows_nt<C>()>(O, 0, obs + e0 * (int64_t)(4 * qe), nenv, qe, tid);
  } else {
    if (stepped) {
      if constexpr (ORDERED)
        run_steps<C, POLICY, ORDERED, PH_ALL>(a, s, L, k, gid, e, tid, &OK.k[0][0]);
      else
        run_steps<C, POLICY, ORDERED, PH_ALL>(a, s, L, k, gid, e, tid);
      store_env<C>(s, L, a.state, a.B, e0, na, tid);
    }
    if (loaded) write_image<C>(s, L, O, tid, na, 0);
    __syncthreads();
    write_rows<C, rows_nt<C>()>(O, 0, obs + e0 * (int64_t)(4 * qe), nenv, qe, tid);
  }
}
