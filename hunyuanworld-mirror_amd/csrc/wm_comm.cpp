// The communicator of the sharded forward: RCCL, or the in-process group of the tests; its all-gather and its communication queue.
#include "wm_model.h"

namespace wm_host {

// ---------------------------------------------------------------- collective
wm_status comm_allgather(wm_handle* h, const void* send, void* recv, size_t bytes, hipStream_t s) {
  ProfScope ps(h, PK_COMM, s);   // the collective, on the queue it runs on (the compute queue unless tuning comm_overlap = 1)
  Comm& cm = h->comm;
  if (cm.kind == 1) {
    if (wm_tune(WM_TUNE_COMM_P2P, 0) == 1) {
      // Direct all-gather (opt-in, tuning comm_p2p = 1 / bench.py --gather p2p): every rank sends its chunk to every peer and
      // receives every peer's chunk as ONE group of point-to-point operations, so each of the 7 xGMI links of a GPU carries one
      // chunk in each direction at once (~0.29 ms per layer link-bound at C4, against ~2.1 ms if the all-gather
      // runs as a ring).  Not the default: no multi-GPU node was available to any build round, and RCCL may already pick a
      // direct algorithm for ncclAllGather on a fully connected node — the first 8-GPU run has to say.
      if (ncclGroupStart() != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclGroupStart failed");
      for (int r = 0; r < cm.world; ++r) {
        if (r == cm.rank) continue;
        if (ncclSend(send, bytes, ncclInt8, r, cm.nccl, s) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclSend failed");
        if (ncclRecv((char*)recv + (size_t)r * bytes, bytes, ncclInt8, r, cm.nccl, s) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclRecv failed");
      }
      if (ncclGroupEnd() != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclGroupEnd failed");
      HIPCHK(h, hipMemcpyAsync((char*)recv + (size_t)cm.rank * bytes, send, bytes, hipMemcpyDeviceToDevice, s));
      return WM_OK;
    }
    if (ncclAllGather(send, recv, bytes, ncclInt8, cm.nccl, s) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclAllGather failed");
    return WM_OK;
  }
  if (cm.kind == 2) {
    wm_local_group* g = cm.grp;
    g->recv[cm.rank] = recv;
    HIPCHK(h, hipStreamSynchronize(s));
    pthread_barrier_wait(&g->bar);
    for (int r = 0; r < g->world; ++r)
      HIPCHK(h, hipMemcpyAsync((char*)g->recv[r] + (size_t)cm.rank * bytes, send, bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
    pthread_barrier_wait(&g->bar);
    return WM_OK;
  }
  return fail(h, WM_ERR_COMM, "sharded forward without a communicator");
}

namespace {
// The communication queue of the overlapped K/V gather (backbone_block) belongs to the communicator: created with it, once per handle, for a
// world of more than one rank; destroyed by wm_destroy.  A communicator may be attached after wm_reserve.
wm_status create_comm_queue(wm_handle* h) {
  if (h->comm.world <= 1) return WM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->cstream) HIPCHK(h, hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking));
  if (!h->cfork) HIPCHK(h, hipEventCreateWithFlags(&h->cfork, hipEventDisableTiming));
  if (!h->cjoin) HIPCHK(h, hipEventCreateWithFlags(&h->cjoin, hipEventDisableTiming));
  return WM_OK;
}
}  // namespace

}  // namespace wm_host
using namespace wm_host;

// ====================================================================================== communicator
extern "C" wm_status wm_rccl_unique_id(uint8_t id[WM_RCCL_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= WM_RCCL_ID_BYTES, "id buffer too small");
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return WM_ERR_COMM;
  memset(id, 0, WM_RCCL_ID_BYTES);
  memcpy(id, &u, sizeof(u));
  return WM_OK;
}

extern "C" wm_status wm_comm_init_rccl(wm_handle* h, const uint8_t id[WM_RCCL_ID_BYTES], int rank, int world) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return WM_ERR_INVALID;
  HIPCHK(h, hipSetDevice(h->device));
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  if (ncclCommInitRank(&h->comm.nccl, world, u, rank) != ncclSuccess) return fail(h, WM_ERR_COMM, "ncclCommInitRank failed");
  h->comm.kind = 1; h->comm.rank = rank; h->comm.world = world;
  return create_comm_queue(h);
}

extern "C" wm_local_group* wm_local_group_create(int world) {
  wm_local_group* g = new wm_local_group();
  g->world = world;
  g->recv.assign(world, nullptr);
  pthread_barrier_init(&g->bar, nullptr, world);
  return g;
}
extern "C" void wm_local_group_destroy(wm_local_group* g) {
  if (!g) return;
  pthread_barrier_destroy(&g->bar);
  delete g;
}
extern "C" wm_status wm_comm_init_local(wm_handle* h, wm_local_group* g, int rank) {
  if (!h || !g || rank < 0 || rank >= g->world) return WM_ERR_INVALID;
  h->comm.kind = 2; h->comm.rank = rank; h->comm.world = g->world; h->comm.grp = g;
  return create_comm_queue(h);
}

extern "C" wm_status wm_allgather(wm_handle* h, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
  if (!h || !send || !recv || bytes_per_rank == 0) return WM_ERR_INVALID;
  return comm_allgather(h, send, recv, bytes_per_rank, (hipStream_t)stream);
}
