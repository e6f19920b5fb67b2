// Host-side glue of mpcb_solve_iterate_pw17 / mpcb_solve_vjp_pw17 under AddressSanitizer, without a
// device: this program is the C API's translation unit itself (included below) with CPU stubs in
// place of the two PW launchers and of the three HIP runtime calls the entry points make.  The stubs
// do on the host what the kernels do with the weight arguments: for every instance of every chunk
// they read the 17x17 / 6x6 / 17x17 records at base + b * stride, from the clamped b for a ragged
// wave's padding groups.  The weight arrays are heap blocks of exactly (B - 1) * stride + record
// elements, so a read of a pad past the last record, a stride applied to a NULL fallback or a
// chunk offset applied twice is an ASan report.  Build and run: tools/asan_pw17.sh.
//
// What must be stubbed.  The program links with --unresolved-symbols=ignore-all, because the C API's
// other entry points refer to launchers that are never called here; a launcher that IS called and
// has no stub below would be a call through a null address, not a link error.  The two entry points
// under test call exactly launch_full17_pw, launch_vjp17_pw and launch_vjp17 (the product with all
// weight pointers NULL), and of the HIP runtime hipSetDevice and hipMalloc (ensure_vjp17_ws): when
// pw17_impl, vjp17_impl or the two entry points in mpcb_capi.hip come to call anything else, add its
// stub here.  The handle is built by hand with the fields those paths read (cfg, device, max_batch,
// full, chunk, weights, params, vjp17_scratch), as tools/asan/capi_host.c cannot create one without
// a device.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mpc_blaster_amd/csrc/mpcb_capi.hip"

// ---- HIP runtime stubs (no device here; the executable's definitions win over the runtime's)
extern "C" hipError_t hipSetDevice(int) { return hipSuccess; }
extern "C" hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
extern "C" hipError_t hipFree(void* p) { free(p); return hipSuccess; }

// ---- launcher stubs
namespace {
struct Seen { long launches = 0, instances = 0, pw = 0; double sum = 0; } g_seen;

template <class T> void read_weights(const Pw17<T>& pw, int64_t b0, int64_t nb) {
  const int64_t groups = (nb + 3) / 4 * 4;   // whole waves: the padding groups read the last instance's
  for (int64_t c = 0; c < groups; ++c) {
    const int64_t b = b0 + (c < nb ? c : nb - 1);
    const T *Q = pw.Q + b * pw.Q_sb, *R = pw.R + b * pw.R_sb, *QN = pw.QN + b * pw.QN_sb;
    for (int e = 0; e < NX17 * NX17; ++e) g_seen.sum += (double)Q[e] + (double)QN[e];
    for (int e = 0; e < NU17 * NU17; ++e) g_seen.sum += (double)R[e];
  }
}
}  // namespace

namespace mpcb {
template <class T> hipError_t launch_full17_pw(const FullArgs<T>& a, const Pw17<T>* pw, hipStream_t) {
  ++g_seen.launches;
  g_seen.instances += a.nb;
  if (a.qp_stats) return hipErrorInvalidValue;   // the PW call never writes the statistics
  if (pw) { ++g_seen.pw; read_weights(*pw, a.b0, a.nb); }
  return hipSuccess;
}
template <class T> hipError_t launch_vjp17_pw(const Vjp17Args<T>& a, const Pw17<T>& pw, hipStream_t) {
  ++g_seen.launches;
  ++g_seen.pw;
  g_seen.instances += a.nb;
  read_weights(pw, a.b0, a.nb);
  return hipSuccess;
}
template <class T> hipError_t launch_vjp17(const Vjp17Args<T>& a, hipStream_t) {
  ++g_seen.launches;
  g_seen.instances += a.nb;
  return hipSuccess;
}
template hipError_t launch_full17_pw<double>(const FullArgs<double>&, const Pw17<double>*, hipStream_t);
template hipError_t launch_full17_pw<float>(const FullArgs<float>&, const Pw17<float>*, hipStream_t);
template hipError_t launch_vjp17_pw<double>(const Vjp17Args<double>&, const Pw17<double>&, hipStream_t);
template hipError_t launch_vjp17_pw<float>(const Vjp17Args<float>&, const Pw17<float>&, hipStream_t);
template hipError_t launch_vjp17<double>(const Vjp17Args<double>&, hipStream_t);
template hipError_t launch_vjp17<float>(const Vjp17Args<float>&, hipStream_t);
}  // namespace mpcb

#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s (last error: %s)\n", __LINE__, #c, mpcb_last_error()); return 1; } } while (0)

// an exact-size heap block of a weight argument: B records at the stride (one record for stride 0)
template <class T> std::vector<T>* block(int64_t B, int64_t stride, int rec) {
  return new std::vector<T>((size_t)((stride ? (B - 1) * stride : 0) + rec), T(1));
}

template <class T> int run(int dtype) {
  const int64_t B = 70;
  const int N = 6;
  mpcb_handle* h = new mpcb_handle();
  h->cfg = mpcb_config{};
  h->cfg.nx = 17; h->cfg.nu = 6; h->cfg.N = N; h->cfg.dtype = dtype; h->cfg.dt = 1.0 / 30; h->cfg.cost_scale = 1.0 / 30;
  h->device = 0;
  h->max_batch = B;
  h->full = 1;
  h->chunk = 64;   // chunks of 64 and 6: the second ends in a ragged wave
  Weights17<T>* W = new Weights17<T>();
  for (T& v : W->Q) v = T(2);
  for (T& v : W->R) v = T(3);
  for (T& v : W->QN) v = T(4);
  h->weights = W;
  h->scratch = nullptr;   // (the stub reads no workspace)
  // required arrays: the glue only passes them on, one element each is enough to be non-null
  T one[1] = {T(0)};
  int32_t st[1] = {0};
  const int QR = NX17 * NX17, RR = NU17 * NU17;
  auto solve = [&](const void* Q, int64_t qs, const void* R, int64_t rs, const void* QN, int64_t qns) {
    return mpcb_solve_iterate_pw17(h, B, one, 17, one, one, one, 0, one, 0, Q, qs, R, rs, QN, qns, one, nullptr, nullptr,
                                   st, nullptr);
  };
  auto vjp = [&](const void* Q, int64_t qs, const void* R, int64_t rs, const void* QN, int64_t qns) {
    return mpcb_solve_vjp_pw17(h, B, one, one, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, Q, qs, R, rs, QN, qns,
                               one, nullptr, one, nullptr, nullptr, nullptr, nullptr, nullptr, st, nullptr);
  };
  // packed, padded and broadcast arrays; a NULL among them falls back to the handle's matrix with
  // stride 0 whatever stride came with it
  for (int64_t pad : {0, 5, 1000}) {
    auto *Q = block<T>(B, QR + pad, QR), *R = block<T>(B, RR + pad, RR), *QN = block<T>(B, QR + pad, QR);
    g_seen = Seen{};
    CHECK(solve(Q->data(), QR + pad, R->data(), RR + pad, QN->data(), QR + pad) == MPCB_OK);
    CHECK(g_seen.launches == 2 && g_seen.pw == 2 && g_seen.instances == B);
    CHECK(g_seen.sum == (64 + 8) * (2.0 * QR + RR));   // 64 + (6 -> 8 groups) records of ones
    g_seen = Seen{};
    CHECK(vjp(Q->data(), QR + pad, R->data(), RR + pad, QN->data(), QR + pad) == MPCB_OK);
    CHECK(g_seen.launches == 2 && g_seen.pw == 2 && g_seen.instances == B);
    g_seen = Seen{};
    CHECK(solve(Q->data(), QR + pad, nullptr, 12345, nullptr, 777) == MPCB_OK);   // R, QN: the handle's
    CHECK(g_seen.sum == (64 + 8) * (1.0 * QR + 3.0 * RR + 4.0 * QR));
    g_seen = Seen{};
    CHECK(vjp(nullptr, 99, R->data(), RR + pad, nullptr, 0) == MPCB_OK);
    CHECK(g_seen.sum == (64 + 8) * (2.0 * QR + 1.0 * RR + 4.0 * QR));
    delete Q; delete R; delete QN;
  }
  {
    auto *Q = block<T>(B, 0, QR), *R = block<T>(B, 0, RR), *QN = block<T>(B, 0, QR);   // stride 0: one record each
    g_seen = Seen{};
    CHECK(solve(Q->data(), 0, R->data(), 0, QN->data(), 0) == MPCB_OK && g_seen.pw == 2);
    CHECK(vjp(Q->data(), 0, R->data(), 0, QN->data(), 0) == MPCB_OK);
    // all three NULL: the shared-weight launchers (no Pw17 at all)
    g_seen = Seen{};
    CHECK(solve(nullptr, 0, nullptr, 0, nullptr, 0) == MPCB_OK && g_seen.launches == 2 && g_seen.pw == 0);
    CHECK(vjp(nullptr, 0, nullptr, 0, nullptr, 0) == MPCB_OK && g_seen.launches == 4 && g_seen.pw == 0);
    // refusals launch nothing
    g_seen = Seen{};
    CHECK(solve(Q->data(), -1, R->data(), 0, QN->data(), 0) == MPCB_E_INVALID);
    CHECK(solve(Q->data(), 0, R->data(), -1, QN->data(), 0) == MPCB_E_INVALID);
    CHECK(vjp(Q->data(), 0, R->data(), 0, QN->data(), -1) == MPCB_E_INVALID);
    CHECK(mpcb_solve_iterate_pw17(h, B + 1, one, 17, one, one, one, 0, one, 0, Q->data(), 0, nullptr, 0, nullptr, 0, one,
                                  nullptr, nullptr, st, nullptr) == MPCB_E_INVALID);
    CHECK(mpcb_solve_iterate_pw17(h, B, one, 17, nullptr, one, one, 0, one, 0, Q->data(), 0, nullptr, 0, nullptr, 0, one,
                                  nullptr, nullptr, st, nullptr) == MPCB_E_INVALID);
    CHECK(mpcb_solve_iterate_pw17(h, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0,
                                  nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == MPCB_OK);   // B = 0
    h->cfg.box_x = 1;
    CHECK(vjp(Q->data(), 0, R->data(), 0, QN->data(), 0) == MPCB_E_UNSUPPORTED);
    h->cfg.box_x = 0;
    h->full = 0;
    CHECK(solve(Q->data(), 0, R->data(), 0, QN->data(), 0) == MPCB_E_UNSUPPORTED);
    CHECK(vjp(Q->data(), 0, R->data(), 0, QN->data(), 0) == MPCB_E_UNSUPPORTED);
    h->full = 1;
    CHECK(g_seen.launches == 0);
    delete Q; delete R; delete QN;
  }
  free(h->vjp17_scratch);
  delete W;
  delete h;
  return 0;
}

int main() {
  if (run<double>(MPCB_F64)) return 1;
  if (run<float>(MPCB_F32)) return 1;
  printf("pw17_glue_clean\n");
  return 0;
}
