// pack.h -- canonical <-> packed state (device code; included by warehouse_amd.hip after
// device_vocab.h): k_pack and k_unpack, runtime dimensions, not on the hot path.  Delivery index <->
// cell is geometry.h's (included by warehouse_amd.hip ahead of the namespace).
// canonical <-> packed (runtime dims; not on the hot path)
struct PackParams {
  uint32_t* state;
  const uint32_t* cstate;
  int64_t B;
  int32_t na, P, pw, D;
  int32_t *pos, *agent_target, *pickup_target, *pickup_timer, *t, *n;
  uint8_t* fresh;
  uint32_t* episode;
};

__global__ __launch_bounds__(BT) void k_pack(PackParams a) {
  const int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (e >= a.B) return;
  const int64_t B = a.B;
  // out-of-range canonical values are clamped so packed state always indexes inside the grid
  const uint32_t n = min((uint32_t)max(a.n[e], 0), (uint32_t)a.na);
  a.state[e] = ((uint32_t)a.t[e] & 0xFFFFu) | (n << 16) | (a.fresh[e] ? (1u << 24) : 0u);
  a.state[B + e] = a.episode[e];
  const int32_t DP = 4 * (a.D - 4);
  for (int i = 0; i < a.na; ++i) {
    uint32_t w = IDLE;
    if (i < (int)n) {
      const int32_t tg = a.agent_target[e * a.na + i];
      const uint32_t x = (uint32_t)min(max(a.pos[(e * a.na + i) * 2], 0), a.D - 1);
      const uint32_t y = (uint32_t)min(max(a.pos[(e * a.na + i) * 2 + 1], 0), a.D - 1);
      uint32_t target = IDLE;
      if (tg >= 0 && tg < DP) {
        const wh_geo::Cell c = wh_geo::delivery_cell(tg, a.D);
        target = ((uint32_t)c.x << 8) | ((uint32_t)c.y << 24);
      }
      w = x | (y << 16) | target;
    }
    a.state[(2 + i) * B + e] = w;
  }
  for (int w = 0; w < a.pw; ++w) {
    uint32_t tw = 0, mw = 0;
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * w + b;
      const int32_t tg = a.pickup_target[e * a.P + j];
      if (tg >= 0 && tg < DP) {
        tw |= (uint32_t)(tg + 1) << (8 * b);
        mw |= (((uint32_t)a.t[e] + (uint32_t)a.pickup_timer[e * a.P + j]) & 0xFFu) << (8 * b);   // expiry step
      }
    }
    a.state[(2 + a.na + w) * B + e] = tw;
    a.state[(2 + a.na + a.pw + w) * B + e] = mw;
  }
}

__global__ __launch_bounds__(BT) void k_unpack(PackParams a) {
  const int64_t e = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (e >= a.B) return;
  const int64_t B = a.B;
  const uint32_t h = a.cstate[e];
  const uint32_t n = (h >> 16) & 0xFFu;
  a.t[e] = (int32_t)(h & 0xFFFFu);
  a.n[e] = (int32_t)n;
  a.fresh[e] = (uint8_t)((h >> 24) & 1u);
  a.episode[e] = a.cstate[B + e];
  for (int i = 0; i < a.na; ++i) {
    const uint32_t w = a.cstate[(2 + i) * B + e];
    const bool live = i < (int)n;
    a.pos[(e * a.na + i) * 2] = live ? (int32_t)(w & 0xFFu) : 0;
    a.pos[(e * a.na + i) * 2 + 1] = live ? (int32_t)((w >> 16) & 0xFFu) : 0;
    const bool carry = live && (w & 0xFF00u) != 0xFF00u;
    a.agent_target[e * a.na + i] = carry ? wh_geo::delivery_index((int)((w >> 8) & 0xFFu), (int)(w >> 24), a.D) : -1;
  }
  for (int w = 0; w < a.pw; ++w) {
    const uint32_t tw = a.cstate[(2 + a.na + w) * B + e];
    const uint32_t mw = a.cstate[(2 + a.na + a.pw + w) * B + e];
    for (int b = 0; b < 4; ++b) {
      const int j = 4 * w + b;
      const uint32_t tg = (tw >> (8 * b)) & 0xFFu;
      a.pickup_target[e * a.P + j] = (int32_t)tg - 1;
      a.pickup_timer[e * a.P + j] = tg ? (int32_t)(((mw >> (8 * b)) - h) & 0xFFu) : -1;   // steps left
    }
  }
}
