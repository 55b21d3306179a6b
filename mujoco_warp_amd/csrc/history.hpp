// Actuator and sensor delays (reference history.py): ring buffers of past ctrl / sensor values in Data.history [nworld, nhistory].
//
// A buffer is [user, cursor, times[n], values[n * dim]] at *_historyadr (dim 1 for an actuator, sensor_dim for a sensor; actuator buffers
// first, then sensor buffers, in id order).  cursor is the PHYSICAL index of the newest sample; logical index i (0 = oldest) lives at
// (cursor + 1 + i) % n; times increase with the logical index.
//   read at t    clamp to the oldest / newest sample within 1e-6 s, an exact match within 1e-6 s returns that sample, otherwise the samples
//                around t are found by the circular binary search and interpolated: 0 zero-order hold, 1 linear, 2 cubic Hermite with
//                Catmull-Rom slopes (zero at the buffer's ends) -- history.py:77-152
//   insert at t  an exact match overwrites, older than the oldest replaces the oldest, newer than the newest advances the cursor, anything
//                else shifts the older samples down and inserts -- history.py:255-302
// Every buffer is owned by exactly one lane of a launch: no atomics, no barriers, results bitwise reproducible and independent of nworld.
// Lanes are flat over (world, actuator | listed sensor) with the world slowest: a wavefront's buffers are neighbours in one or two rows of
// Data.history.  The work per lane is a handful of dependent loads; the branches (which of the four insert cases, which interpolation)
// are uniform over the worlds of a model that steps in lockstep.
// A read and an insert of the same step are ONE pass (hist_step): the samples around the read time and the insert's target slot are decided
// first, from the times as they are; then, component by component, the delayed value is read before the fresh one is stored (the target
// slot may be the oldest sample, the very one the read returns: nsample 1 or 2); the slot's time and the cursor are written last.
#pragma once
#include "dev_common.hpp"

#define HIST_EPS 1e-6f
#define HIST_NOTIME -1e10f  // (-mjMAXVAL: the time of samples initialised without times, history.py:785-790)

DEV int hist_phys(int cursor, int n, int logical) {  // cursor, logical in [0, n)
  const int p = cursor + 1 + logical;
  return p >= n ? p - n : p;
}
// the cursor as stored (a float; a Data.history copied in from elsewhere is not trusted to be in range)
DEV int hist_cursor(const float* buf, int n) { return min(max((int)buf[1], 0), n - 1); }

// logical index i with times[i - 1] < t <= times[i]: 0 if t <= the oldest time, n if t > the newest (history.py:33-73)
DEV int hist_find(const float* times, int n, int cursor, float t) {
  if (t <= times[hist_phys(cursor, n, 0)]) return 0;
  if (t > times[hist_phys(cursor, n, n - 1)]) return n;
  int lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (times[hist_phys(cursor, n, mid)] < t) lo = mid;
    else hi = mid;
  }
  return hi;
}

// what a read at t needs, decided once per buffer: the physical samples around t and the weights (the same for every component)
struct HistSpan {
  int mode;  // 0: the sample `hi` as it is (clamped or exact), 1: the sample `lo` (zero-order hold), 2: linear, 3: cubic
  int lo, hi, prev, next;  // physical indices; prev / next -1 at the buffer's ends (zero slope)
  float alpha, dt, dt_lo, dt_hi;
};
DEV HistSpan hist_span(const float* buf, int n, int cursor, float t, int interp) {
  const float* times = buf + 2;
  HistSpan sp{0, 0, 0, -1, -1, 0.0f, 0.0f, 0.0f, 0.0f};
  const int oldest = hist_phys(cursor, n, 0), newest = hist_phys(cursor, n, n - 1);
  if (t <= times[oldest] + HIST_EPS) {
    sp.hi = oldest;
    return sp;
  }
  if (t >= times[newest] - HIST_EPS) {
    sp.hi = newest;
    return sp;
  }
  // (oldest + eps < t < newest - eps: n >= 2 and 1 <= i <= n - 1)
  const int i = hist_find(times, n, cursor, t);
  sp.hi = hist_phys(cursor, n, i);
  const float t_hi = times[sp.hi];
  if (fabsf(t - t_hi) < HIST_EPS) return sp;
  sp.lo = hist_phys(cursor, n, i - 1);
  const float t_lo = times[sp.lo];
  if (interp == 0) {
    sp.mode = 1;
    return sp;
  }
  sp.dt = t_hi - t_lo;
  sp.alpha = (t - t_lo) / sp.dt;
  if (interp == 1) {
    sp.mode = 2;
    return sp;
  }
  sp.mode = 3;
  if (i > 1) {
    sp.prev = hist_phys(cursor, n, i - 2);
    sp.dt_lo = t_hi - times[sp.prev];
  }
  if (i < n - 1) {
    sp.next = hist_phys(cursor, n, i + 1);
    sp.dt_hi = times[sp.next] - t_lo;
  }
  return sp;
}
// component c of the buffer's value at the span's time (values: buf + 2 + n)
DEV float hist_read(const float* values, int dim, int c, const HistSpan& sp) {
  const float v_hi = values[sp.hi * dim + c];
  if (sp.mode == 0) return v_hi;
  const float v_lo = values[sp.lo * dim + c];
  if (sp.mode == 1) return v_lo;
  const float a = sp.alpha;
  if (sp.mode == 2) return v_lo + a * (v_hi - v_lo);
  const float a2 = a * a, a3 = a2 * a;
  const float h00 = 2.0f * a3 - 3.0f * a2 + 1.0f, h10 = a3 - 2.0f * a2 + a, h01 = -2.0f * a3 + 3.0f * a2, h11 = a3 - a2;
  const float m_lo = sp.prev >= 0 ? (v_hi - values[sp.prev * dim + c]) / sp.dt_lo : 0.0f;
  const float m_hi = sp.next >= 0 ? (values[sp.next * dim + c] - v_lo) / sp.dt_hi : 0.0f;
  return h00 * v_lo + h10 * sp.dt * m_lo + h01 * v_hi + h11 * sp.dt * m_hi;
}

// where an insert at t goes, decided without writing anything
struct HistSlot {
  int slot;     // physical sample that takes the new value
  int nshift;   // out-of-order insert: logical samples 1 .. nshift move down by one first (0 otherwise)
  int cursor;   // the cursor after the insert
  bool exact;   // the sample exists already: only its value is written
};
DEV HistSlot hist_insert_slot(const float* buf, int n, int cursor, float t) {
  const float* times = buf + 2;
  const int i = hist_find(times, n, cursor, t);
  if (i < n) {
    const int p = hist_phys(cursor, n, i);
    if (fabsf(t - times[p]) < HIST_EPS) return HistSlot{p, 0, cursor, true};
  }
  if (i == 0) return HistSlot{hist_phys(cursor, n, 0), 0, cursor, false};  // older than the oldest: replaces it
  if (i == n) {                                                            // newer than the newest: the cursor advances onto the oldest
    const int c1 = cursor + 1 >= n ? 0 : cursor + 1;
    return HistSlot{c1, 0, c1, false};
  }
  return HistSlot{hist_phys(cursor, n, i - 1), i - 1, cursor, false};  // in between: samples 1 .. i - 1 move down, the oldest goes
}
// component c of the insert: the shift of an out-of-order insert, then the value
DEV void hist_insert(float* values, int n, int dim, int cursor, int c, const HistSlot& sl, float v) {
  for (int j = 0; j < sl.nshift; ++j) values[hist_phys(cursor, n, j) * dim + c] = values[hist_phys(cursor, n, j + 1) * dim + c];
  values[sl.slot * dim + c] = v;
}
// the times and the cursor, after every component
DEV void hist_insert_commit(float* buf, int n, int cursor, const HistSlot& sl, float t) {
  float* times = buf + 2;
  for (int j = 0; j < sl.nshift; ++j) times[hist_phys(cursor, n, j)] = times[hist_phys(cursor, n, j + 1)];
  if (!sl.exact) times[sl.slot] = t;
  if (sl.cursor != cursor) buf[1] = (float)sl.cursor;
}

// One buffer's part of a forward evaluation at time t: out[c] = the buffer read at t - delay (delay > 0) or fresh[c]; then, when asked, fresh is
// inserted at t.  out may be fresh itself (a sensor's slice of sensordata).
DEV void hist_step(float* buf, int n, int dim, float t, float delay, int interp, bool insert, const float* fresh, float* out) {
  const int cursor = hist_cursor(buf, n);
  float* values = buf + 2 + n;
  const bool read = delay > 0.0f;
  HistSpan sp;
  HistSlot sl;
  if (read) sp = hist_span(buf, n, cursor, t - delay, interp);
  if (insert) sl = hist_insert_slot(buf, n, cursor, t);
  for (int c = 0; c < dim; ++c) {
    const float v = fresh[c];
    if (read) out[c] = hist_read(values, dim, c, sp);
    else if (out != fresh) out[c] = v;
    if (insert) hist_insert(values, n, dim, cursor, c, sl, v);
  }
  if (insert) hist_insert_commit(buf, n, cursor, sl, t);
}

// Data.ws_ctrl_delayed [nworld, nu] = what the actuation stage reads as ctrl at Data.time: the actuator's buffer read at time - delay
// (nsample > 0 and delay > 0), ctrl otherwise; insert != 0 (a step, once, at its own start time) then stores (time, ctrl) in every buffer.
// One lane per (world, actuator).
__global__ void __launch_bounds__(256) k_history_ctrl(MjhModel m, MjhData d, const float* ctrl, int insert) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= d.nworld * m.nu) return;
  const int w = idx / m.nu, u = idx - w * m.nu;
  const int n = m.actuator_history[2 * u];
  if (n <= 0) {
    d.ws_ctrl_delayed[idx] = ctrl[idx];
    return;
  }
  float* buf = d.history + (size_t)w * m.nhistory + m.actuator_historyadr[u];
  hist_step(buf, n, 1, d.time[w], m.actuator_delay[u], m.actuator_history[2 * u + 1], insert != 0, ctrl + idx, d.ws_ctrl_delayed + idx);
}

// Behind a sensor launch: every sensor of that stage with nsample > 0 (ids: the model's list of the stage, nlist entries) replaces its slice
// of sensordata by the buffer read at time - delay (delay > 0) and, when asked, stores the fresh values at time.  One lane per (world, listed sensor).
__global__ void __launch_bounds__(256) k_history_sensor(MjhModel m, MjhData d, const int* list, int nlist, int insert) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= d.nworld * nlist) return;
  const int w = idx / nlist, i = list[idx - w * nlist];
  const int n = m.sensor_history[2 * i];
  if (n <= 0) return;
  float* buf = d.history + (size_t)w * m.nhistory + m.sensor_historyadr[i];
  float* sd = d.sensordata + (size_t)w * m.nsensordata + m.sensor_adr[i];
  hist_step(buf, n, m.sensor_dim[i], d.time[w], m.sensor_delay[i], m.sensor_history[2 * i + 1], insert != 0, sd, sd);
}

// read_ctrl / read_sensor: result[w, 0 .. dim) = the buffer of actuator / sensor `id` at time[w] - delay (history.py:601-631, 669-715); interp -1:
// the model's.  Without a buffer: Data.ctrl / Data.sensordata.  One lane per world.
__global__ void __launch_bounds__(256) k_history_read(MjhModel m, MjhData d, int is_sensor, int id, const float* time, int interp, float* result, int stride) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= d.nworld) return;
  const int* hist = (is_sensor ? m.sensor_history : m.actuator_history) + 2 * id;
  const int n = hist[0], dim = is_sensor ? m.sensor_dim[id] : 1;
  float* out = result + (size_t)w * stride;
  if (n <= 0) {
    const float* src = is_sensor ? d.sensordata + (size_t)w * m.nsensordata + m.sensor_adr[id] : d.ctrl + (size_t)w * m.nu + id;
    for (int c = 0; c < dim; ++c) out[c] = src[c];
    return;
  }
  const float* buf = d.history + (size_t)w * m.nhistory + (is_sensor ? m.sensor_historyadr : m.actuator_historyadr)[id];
  const float delay = (is_sensor ? m.sensor_delay : m.actuator_delay)[id];
  const HistSpan sp = hist_span(buf, n, hist_cursor(buf, n), time[w] - delay, interp < 0 ? hist[1] : interp);
  for (int c = 0; c < dim; ++c) out[c] = hist_read(buf + 2 + n, dim, c, sp);
}

// init_ctrl_history / init_sensor_history (history.py:756-793, 841-878): the buffer of `id` in every world = the samples values[w, 0 .. n * dim),
// oldest first, at times[0 .. n) (nullptr: HIST_NOTIME); cursor n - 1; the user slot = phase[w] (nullptr: kept).  One lane per world.
__global__ void __launch_bounds__(256) k_history_init(MjhModel m, MjhData d, int is_sensor, int id, const float* times, const float* values, int stride, const float* phase) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= d.nworld) return;
  const int n = (is_sensor ? m.sensor_history : m.actuator_history)[2 * id], dim = is_sensor ? m.sensor_dim[id] : 1;
  if (n <= 0) return;  // (no buffer: the binding refuses this by name; nothing is written)
  float* buf = d.history + (size_t)w * m.nhistory + (is_sensor ? m.sensor_historyadr : m.actuator_historyadr)[id];
  const float* src = values + (size_t)w * stride;
  if (phase) buf[0] = phase[w];
  buf[1] = (float)(n - 1);
  for (int k = 0; k < n; ++k) buf[2 + k] = times ? times[k] : HIST_NOTIME;
  for (int k = 0; k < n * dim; ++k) buf[2 + n + k] = src[k];
}
