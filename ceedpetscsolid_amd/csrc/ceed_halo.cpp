// ceed_halo.cpp -- the interface sum between element partitions over RCCL (CeedXComm*, CeedXHalo*): the library's
// replacement of DMLocalToGlobal(ADD_VALUES) + DMGlobalToLocal across the GPUs of one node (src/matops.c:33,57,126,153,
// 171,199,238) and of the MPI reductions behind VecDot / VecNorm (CeedXCommAllReduce).
//
// RCCL is bound at first use with dlopen: a C host gets /opt/rocm's librccl, a Python host the copy torch has already
// loaded (one RCCL per process, like the HIP runtime: see ceed.py).  No link-time dependency for single-GPU users.
#include <dlfcn.h>

#include "ceed_impl.hpp"
#include "index_maps.hpp"

using namespace cps;

extern int (*g_rccl_comm_destroy)(void *);   // ceed_core.cpp: the Ceed's destructor ends its communicator through this

namespace {
typedef struct { char internal[128]; } rccl_unique_id;
struct Rccl {
  void *h = nullptr;
  int (*GetUniqueId)(rccl_unique_id *) = nullptr;
  int (*CommInitRank)(void **, int, rccl_unique_id, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*CommCount)(void *, int *) = nullptr;
  int (*CommUserRank)(void *, int *) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
const int RCCL_FLOAT64 = 8;   // ncclFloat64 (rccl.h)
const int RCCL_SUM = 0;       // ncclSum
int rccl_load() {
  if (g_rccl.h) return 0;
  const char *names[] = {"librccl.so.1", "librccl.so"};
  for (int pass = 0; pass < 2 && !g_rccl.h; pass++)      // an already loaded copy first (RTLD_NOLOAD)
    for (const char *n : names)
      if (!g_rccl.h) g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0));
  if (!g_rccl.h) return ceed_error("the halo exchange needs RCCL (librccl.so.1): %s", dlerror());
  auto sym = [](const char *n) { return dlsym(g_rccl.h, n); };
  g_rccl.GetUniqueId = (int (*)(rccl_unique_id *))sym("ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void **, int, rccl_unique_id, int))sym("ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(void *))sym("ncclCommDestroy");
  g_rccl_comm_destroy = g_rccl.CommDestroy;
  g_rccl.CommCount = (int (*)(void *, int *))sym("ncclCommCount");
  g_rccl.CommUserRank = (int (*)(void *, int *))sym("ncclCommUserRank");
  g_rccl.GroupStart = (int (*)())sym("ncclGroupStart");
  g_rccl.GroupEnd = (int (*)())sym("ncclGroupEnd");
  g_rccl.Send = (int (*)(const void *, size_t, int, int, void *, hipStream_t))sym("ncclSend");
  g_rccl.Recv = (int (*)(void *, size_t, int, int, void *, hipStream_t))sym("ncclRecv");
  g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))sym("ncclAllReduce");
  g_rccl.GetErrorString = (const char *(*)(int))sym("ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.Send ||
      !g_rccl.Recv || !g_rccl.AllReduce || !g_rccl.GetErrorString) { g_rccl.h = nullptr; return ceed_error("librccl lacks a point-to-point entry point"); }
  return 0;
}
}  // namespace
#define RCCLCHK(x) do { int r_ = (x); if (r_ != 0) return ceed_error("%s failed: %s", #x, g_rccl.GetErrorString(r_)); } while (0)

extern "C" int CeedXCommGetUniqueId(Ceed, char id[128]) {
  CHK(rccl_load());
  rccl_unique_id u;
  RCCLCHK(g_rccl.GetUniqueId(&u));
  memcpy(id, u.internal, 128);
  return 0;
}
extern "C" int CeedXCommInit(Ceed ceed, int nranks, int rank, const char id[128]) {
  if (ceed->comm) return ceed_error("this Ceed already has a communicator");
  if (nranks < 1 || rank < 0 || rank >= nranks) return ceed_error("CeedXCommInit: rank %d of %d", rank, nranks);
  CHK(rccl_load());
  rccl_unique_id u;
  memcpy(u.internal, id, 128);
  HIPCHK(hipSetDevice(ceed->device));   // (the calling thread's current device may not be the Ceed's)
  RCCLCHK(g_rccl.CommInitRank(&ceed->comm, nranks, u, rank));
  ceed->comm_rank = rank; ceed->comm_size = nranks;
  if (!ceed->comm_stream) {
    // Default priority.  VERDICT r2 asked whether a HIGHEST-priority stream lets RCCL's kernel in beside the persistent
    // fused grid.  Measured on the emulated rank 3 of 8 (profiles/r03_ab_experiments.txt): it does the opposite -- the same
    // exchange alone takes 187-238 us instead of 46-50 us and the whole apply 428-496 us instead of 118 us (the
    // high-priority hardware queue serialises against the compute queues on this part).  CEED_MI355X_COMM_PRIO=1 keeps the A/B.
    int lo = 0, hi = 0;
    if (ceed->opt.comm_priority && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
      HIPCHK(hipStreamCreateWithPriority(&ceed->comm_stream, hipStreamNonBlocking, hi));
    else HIPCHK(hipStreamCreateWithFlags(&ceed->comm_stream, hipStreamNonBlocking));
  }
  return 0;
}
// Ranks in the communicator and this rank's number, READ BACK from RCCL (ncclCommCount / ncclCommUserRank), not the
// values CeedXCommInit was given: what a job reports as "the exchange ran over N ranks" (bench.py: rccl_ranks).  No
// communicator: 0 ranks, rank -1.
extern "C" int CeedXCommGetSize(Ceed ceed, int *nranks, int *rank) {
  if (nranks) *nranks = 0;
  if (rank) *rank = -1;
  if (!ceed->comm) return 0;
  if (!g_rccl.CommCount || !g_rccl.CommUserRank) return ceed_error("librccl lacks ncclCommCount / ncclCommUserRank");
  int n = 0, r = -1;
  RCCLCHK(g_rccl.CommCount(ceed->comm, &n));
  RCCLCHK(g_rccl.CommUserRank(ceed->comm, &r));
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  return 0;
}
extern "C" int CeedXCommDestroy(Ceed ceed) {
  if (ceed->comm) { (void)hipStreamSynchronize(ceed->comm_stream); (void)g_rccl.CommDestroy(ceed->comm); ceed->comm = nullptr; }
  return 0;
}
// Sum of `n` entries of a device vector over all ranks, in place, on the Ceed's stream (the MPI_Allreduce behind VecDot /
// VecNorm, src/matops.c:292 and the Krylov norms): the scalars of a recurrence stay on the device.  One rank: nothing.
extern "C" int CeedXCommAllReduce(Ceed ceed, CeedVector v, CeedInt first, CeedInt n) {
  if (first < 0 || n < 0 || first + n > v->length) return ceed_error("CeedXCommAllReduce: entries [%d, %d) of %d", first, first + n, v->length);
  if (!ceed->comm || ceed->comm_size == 1 || n == 0) return 0;
  double *p;
  CHK(vec_dev(v, true, &p));
  RCCLCHK(g_rccl.AllReduce(p + first, p + first, (size_t)n, RCCL_FLOAT64, RCCL_SUM, ceed->comm, ceed->stream));
  return 0;
}

static void halo_free(CeedXHalo H) {
  if (H->packed) (void)hipEventDestroy(H->packed);
  if (H->arrived) (void)hipEventDestroy(H->arrived);
  Ceed c = H->ceed;
  delete H;            // (before the reference goes: its arrays retire into a Ceed that still exists)
  ceed_unref(c);
}
static int halo_build(CeedXHalo H, CeedInt nneigh, const int *neigh_rank, const CeedInt *count, const CeedInt *const *index) {
  Ceed ceed = H->ceed;
  std::vector<uint32_t> idx;
  for (int k = 0; k < nneigh; k++) {
    if (neigh_rank[k] < 0 || neigh_rank[k] >= ceed->comm_size || count[k] < 0) return ceed_error("CeedXHaloCreate: bad neighbour %d", k);
    HaloNeighbour nb;
    nb.rank = neigh_rank[k]; nb.n = count[k]; nb.offset = (int)idx.size();
    for (int i = 0; i < nb.n; i++) {
      if (index[k][i] < 0) return ceed_error("CeedXHaloCreate: negative index");
      idx.push_back((uint32_t)index[k][i]);
      H->lsize_min = std::max(H->lsize_min, index[k][i] + 1);
    }
    H->nb.push_back(nb);
  }
  H->total = (int)idx.size();
  H->h_idx = idx;
  const HaloArrivals A = halo_arrivals(idx);     // arrivals by destination entry (index_maps.hpp)
  H->ndst = (int)A.dst.size();
  CHK(H->d_idx.upload(ceed, idx)); CHK(H->d_dst.upload(ceed, A.dst)); CHK(H->d_uptr.upload(ceed, A.uptr)); CHK(H->d_uslot.upload(ceed, A.uslot));
  CHK(H->send.alloc(ceed, idx.size())); CHK(H->recv.alloc(ceed, idx.size()));
  HIPCHK(hipEventCreateWithFlags(&H->packed, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&H->arrived, hipEventDisableTiming));
  return 0;
}
// Neighbour lists: `index[k]` holds the `count[k]` L-vector entries shared with rank `neigh_rank[k]`, in an order both
// sides agree on (halo.py sorts them by partition-independent node keys).  Entries are unique within one list.
extern "C" int CeedXHaloCreate(Ceed ceed, CeedInt nneigh, const int *neigh_rank, const CeedInt *count,
                               const CeedInt *const *index, CeedXHalo *halo) {
  if (nneigh > 0 && !ceed->comm) return ceed_error("CeedXHaloCreate: call CeedXCommInit first");
  static long n_created = 0;
  CeedXHalo H = new CeedXHalo_private;
  H->ceed = ceed; ceed_ref(ceed);
  H->serial = ++n_created;
  const int ierr = halo_build(H, nneigh, neigh_rank, count, index);
  if (ierr) { halo_free(H); return ierr; }   // nothing of a half-built exchange survives an error return
  *halo = H;
  return 0;
}
// pack on `pack_stream` (the stream that produced y), then all sends and receives of this rank as ONE RCCL group.
// Where the group runs (CeedOptions::comm_inline):
//  * inline (default): on `pack_stream` itself, in order behind the pack kernel -- no event, no second queue.  Measured on
//    the emulated rank 3 of 8 (profiles/r03_rank_of_8_*): every hand-over between two streams costs 10-16 us on this
//    part (a kernel behind hipStreamWaitEvent starts that long after the event's kernel ended), more than the 13 us the
//    RCCL kernel itself takes, and RCCL's 256-thread workgroups do not get a slot beside the fused kernel's resident
//    single-wave workgroups anyway: they start when those retire.  In order on one stream the exchange takes ~25 us
//    instead of ~45.
//  * on the communicator's stream (CEED_MI355X_COMM_INLINE=0): the round-2 form; H->arrived is recorded behind the group
//    and whoever needs the arrivals waits for it.
int halo_pack_and_send(CeedXHalo H, const double *py, hipStream_t pack_stream) {
  Ceed c = H->ceed;
  HIPCHK(launch_halo_pack(H->d_idx.get(), H->total, py, H->send.get(), pack_stream));
  return halo_send(H, pack_stream);
}
// the RCCL group alone: the send buffer has been filled on `pack_stream` (by k_halo_pack or by the rows' launch, HaloPackFold)
int halo_send(CeedXHalo H, hipStream_t pack_stream) {
  Ceed c = H->ceed;
  // Recording into a hipGraph (RCCL 2.26.6 / HIP runtime as shipped with this image's torch): the group issued IN ORDER on the
  // capturing stream records and replays correctly.  Issued on the communicator's stream, joined to the capture by events, the
  // PROCESS dies -- cause established in round 4 (profiles/r04_rccl_capture_probe.txt): not in RCCL's kernels but at
  // hipStreamEndCapture, a stack overflow in libamdhip64.so's self-recursive reset of a capture's forked streams
  // (hip::Stream::EndCapture walking parallelCaptureStreams_: the frame libamdhip64.so+0x2d34a8 repeated until the guard page).
  // RCCL forks an internal stream from the stream it is called on; called on a stream that is itself a fork of the capturing
  // stream, the runtime's lists of forked streams no longer form a tree.  Nothing this library can repair from outside: the form is
  // refused while recording, unconditionally (the CEED_MI355X_HALO_CAPTURE override of round 3 is gone).
  if (c->capturing && !c->opt.comm_inline)
    return ceed_error("the halo exchange on a stream of its own (CEED_MI355X_COMM_INLINE=0) cannot be recorded into a hipGraph: hipStreamEndCapture "
                      "overflows its stack on the forked streams RCCL adds (profiles/r04_rccl_capture_probe.txt); the default in-order form can");
  hipStream_t cs = c->opt.comm_inline ? pack_stream : c->comm_stream;
  if (cs != pack_stream) {
    HIPCHK(hipEventRecord(H->packed, pack_stream));
    HIPCHK(hipStreamWaitEvent(cs, H->packed, 0));
  }
  RCCLCHK(g_rccl.GroupStart());
  for (HaloNeighbour &nb : H->nb) {
    RCCLCHK(g_rccl.Send(H->send.get() + nb.offset, (size_t)nb.n, RCCL_FLOAT64, nb.rank, c->comm, cs));
    RCCLCHK(g_rccl.Recv(H->recv.get() + nb.offset, (size_t)nb.n, RCCL_FLOAT64, nb.rank, c->comm, cs));
  }
  RCCLCHK(g_rccl.GroupEnd());
  HIPCHK(hipEventRecord(H->arrived, cs));
  H->arrived_on = cs;
  return 0;
}
int halo_wait_arrivals(CeedXHalo H, hipStream_t s) {
  if (H->arrived_on != s) HIPCHK(hipStreamWaitEvent(s, H->arrived, 0));     // (the same stream: already in order)
  return 0;
}
HaloUnpackArgs halo_unpack_args(CeedXHalo H) { return HaloUnpackArgs{H->d_dst.get(), H->d_uptr.get(), H->d_uslot.get(), H->recv.get(), H->ndst}; }
// Start: pack on the Ceed's stream, then the RCCL group on the communicator's stream -- the Ceed's stream is free for
// the interior elements meanwhile (CeedXOperatorApplyPhase 1).
extern "C" int CeedXHaloStart(CeedXHalo H, CeedVector y) {
  if (H->in_flight) return ceed_error("CeedXHaloStart: an exchange is already in flight");
  if (H->nb.empty()) return 0;
  if (y->length < H->lsize_min) return ceed_error("CeedXHaloStart: vector shorter than the halo's indices");
  double *py;
  CHK(vec_dev(y, false, &py));
  CHK(halo_pack_and_send(H, py, H->ceed->stream));
  H->in_flight = true;
  return 0;
}
// Finish: the Ceed's stream waits for the arrivals and adds them, per entry in neighbour-list order (a node shared by
// three ranks gets its two additions in the same order every time: the sum is reproducible).
extern "C" int CeedXHaloFinish(CeedXHalo H, CeedVector y) {
  if (H->nb.empty()) return 0;
  if (!H->in_flight) return ceed_error("CeedXHaloFinish without CeedXHaloStart");
  Ceed c = H->ceed;
  double *py;
  CHK(vec_dev(y, true, &py));
  CHK(halo_wait_arrivals(H, c->stream));
  HIPCHK(launch_halo_unpack_add(halo_unpack_args(H), py, c->stream));
  H->in_flight = false;
  return 0;
}
extern "C" int CeedXHaloDestroy(CeedXHalo *halo) {
  if (!halo || !*halo) return 0;
  CeedXHalo H = *halo;
  (void)hipStreamSynchronize(H->ceed->stream);
  if (H->ceed->side_stream) (void)hipStreamSynchronize(H->ceed->side_stream);
  if (H->ceed->comm_stream) (void)hipStreamSynchronize(H->ceed->comm_stream);
  halo_free(H);
  *halo = nullptr;
  return 0;
}
