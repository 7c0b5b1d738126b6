// gather_device.cpp — the Device's two frame gathers over the transports of gather.h: its own
// GPUs' shards onto the first (gather_local), then this process's shard to rank 0
// (gather_process).
#include "device.h"

namespace yrt {

// The ctx devices' shards onto ctx[0]: every peer packs its tiles into a slab, the slabs go to
// the first device (RCCL grouped send/recv when the devices are distinct GPUs — one xGMI link
// per peer; hipMemcpyPeerAsync when ncclCommInitAll is unavailable; a device-to-device copy
// when logical shards share a GPU) and are unpacked there. Every wait is bounded by
// gatherTimeout; a timed-out RCCL gather aborts the communicators and later frames use peer
// copies. Returns the YRT_GATHER_* path taken.
int Device::gather_local(const SlabLayout& base, int numTiles) {
  const int N = (int)ctx.size();
  bool distinct = true;
  for (int a = 0; a < N; ++a)
    for (int b = a + 1; b < N; ++b) distinct &= ctx[a]->hipDevice != ctx[b]->hipDevice;
  GpuCtx& g0 = *ctx[0];
  const size_t eb = slab_element_bytes(base.rgb8);
  std::vector<int> tiles(N);
  std::vector<SlabLayout> lay(N, base);
  for (int k = 1; k < N; ++k) {
    GpuCtx& g = *ctx[k];
    lay[k].tileOffset = shardIndex + k * shardCount;
    lay[k].tileStride = shardCount * N;
    tiles[k] = shard_tiles(numTiles, lay[k].tileOffset, lay[k].tileStride);
    HIP_CHECK(hipSetDevice(g.hipDevice));
    g.dSlab.alloc((size_t)std::max(1, tiles[k]) * 256 * eb);
    launch_pack_tiles(g.fbFloat(), g.fbRGB8(), lay[k], tiles[k], g.dSlab.p, g.stream);
    HIP_CHECK(hipSetDevice(g0.hipDevice));
    g0.recvSlabs[k].alloc((size_t)std::max(1, tiles[k]) * 256 * eb);
  }
  const Clock::time_point deadline =
      Clock::now() + std::chrono::microseconds((long long)(gatherTimeout * 1e6));
  auto wait_ctx = [&](int k, const char* phase) {
    HIP_CHECK(hipSetDevice(ctx[k]->hipDevice));
    if (!stream_wait_until(ctx[k]->stream, deadline))
      throw std::runtime_error(std::string("multi-GPU gather: ") + phase + " on HIP device " +
                               std::to_string(ctx[k]->hipDevice) + " timed out after " +
                               std::to_string(gatherTimeout) + " s");
  };
  int path = distinct ? YRT_GATHER_RCCL_LOCAL : YRT_GATHER_D2D;
  if (distinct && !localRcclOff && !localComm) {
    try {
      const RcclApi& nc = rccl();
      std::vector<int> devs;
      for (auto& g : ctx) devs.push_back(g->hipDevice);
      std::vector<ncclComm_t> comms(N);
      rccl_check(nc.CommInitAll(comms.data(), N, devs.data()), "ncclCommInitAll");
      localComms.assign(comms.begin(), comms.end());
      localComm = comms[0];
    } catch (const std::exception& e) {
      localRcclOff = true;
      localRcclWhy = e.what();
      fprintf(stderr, "yrt: %s; the multi-GPU gather uses hipMemcpyPeerAsync instead\n", e.what());
    }
  }
  if (distinct && localRcclOff) path = YRT_GATHER_PEER_COPY;
  if (path == YRT_GATHER_RCCL_LOCAL) {
    const RcclApi& nc = rccl();
    rccl_check(nc.GroupStart(), "ncclGroupStart");
    for (int k = 1; k < N; ++k) {
      const size_t bytes = (size_t)tiles[k] * 256 * eb;
      if (!bytes) continue;
      rccl_check(nc.Send(ctx[k]->dSlab.p, bytes, ncclUint8, 0, localComms[k], ctx[k]->stream), "ncclSend");
      rccl_check(nc.Recv(g0.recvSlabs[k].p, bytes, ncclUint8, k, localComms[0], g0.stream), "ncclRecv");
    }
    rccl_check(nc.GroupEnd(), "ncclGroupEnd");
  } else {
    for (int k = 1; k < N; ++k) {
      wait_ctx(k, "tile pack");
      const size_t bytes = (size_t)tiles[k] * 256 * eb;
      if (bytes)
        HIP_CHECK(hipMemcpyPeerAsync(g0.recvSlabs[k].p, g0.hipDevice, ctx[k]->dSlab.p, ctx[k]->hipDevice, bytes,
                                     g0.stream));
    }
  }
  HIP_CHECK(hipSetDevice(g0.hipDevice));
  for (int k = 1; k < N; ++k)
    launch_unpack_tiles(g0.recvSlabs[k].p, g0.fbFloat(), g0.fbRGB8(), lay[k], tiles[k],
                        g0.stream);
  try {
    for (int k = 0; k < N; ++k) wait_ctx(k, path == YRT_GATHER_RCCL_LOCAL ? "RCCL slab send/recv" : "slab copy");
  } catch (...) {
    if (path == YRT_GATHER_RCCL_LOCAL) {
      // the communicators may hold a send/recv that never matches: abort them and gather with
      // peer copies from now on
      try {
        const RcclApi& nc = rccl();
        for (auto c : localComms) (nc.CommAbort ? nc.CommAbort : nc.CommDestroy)(c);
      } catch (...) {
      }
      localComms.clear();
      localComm = nullptr;
      localRcclOff = true;
      localRcclWhy = "an RCCL gather timed out";
    }
    throw;
  }
  HIP_CHECK(hipSetDevice(g0.hipDevice));
  return path;
}

// This process's tiles (shard shardIndex of shardCount, already gathered on ctx[0]) to rank 0
// of the process transport (gather.h: RCCL, yrtSetShardComm, or the in-process hub,
// yrtSetShardHub): the ranks first exchange their render status (the min of every rank's
// flag, so a rank whose render failed makes every rank fail instead of leaving rank 0 waiting
// for its slab), then every rank packs its tiles and rank 0 receives each peer's slab and
// unpacks it into its frames. Every wait is bounded: the status exchange by gatherTimeout plus
// kStatusRenderFactor times this rank's render time, the transfers by gatherTimeout.
void Device::gather_process(const SlabLayout& base, int numTiles, bool localOk, double renderSeconds) {
  GpuCtx& g0 = *ctx[0];
  HIP_CHECK(hipSetDevice(g0.hipDevice));
  const int P = shardCount;
  const int flag = proc->exchange_status(localOk ? 1 : 0, g0.hipDevice, g0.stream,
                                         gatherTimeout + kStatusRenderFactor * std::max(0.0, renderSeconds));
  if (!flag) {
    if (localOk) throw std::runtime_error("rtRenderFrame: a peer rank's render failed (no frame gathered)");
    return;  // the caller rethrows this rank's own error
  }
  const size_t eb = slab_element_bytes(base.rgb8);
  SlabLayout L = base;
  L.tileStride = P;
  if (shardIndex != 0) {
    L.tileOffset = shardIndex;
    const int tiles = shard_tiles(numTiles, shardIndex, P);
    g0.dSlab.alloc((size_t)std::max(1, tiles) * 256 * eb);
    launch_pack_tiles(g0.fbFloat(), g0.fbRGB8(), L, tiles, g0.dSlab.p, g0.stream);
    proc->send_root(g0.dSlab.p, (size_t)tiles * 256 * eb, g0.hipDevice, g0.stream, gatherTimeout);
  } else {
    std::vector<int> tiles(P);
    std::vector<void*> bufs(P, nullptr);
    std::vector<size_t> bytes(P, 0);
    for (int r = 1; r < P; ++r) {
      tiles[r] = shard_tiles(numTiles, r, P);
      g0.recvSlabs[r].alloc((size_t)std::max(1, tiles[r]) * 256 * eb);
      bufs[r] = g0.recvSlabs[r].p;
      bytes[r] = (size_t)tiles[r] * 256 * eb;
    }
    proc->recv_all(bufs, bytes, g0.hipDevice, g0.stream, gatherTimeout);
    for (int r = 1; r < P; ++r) {
      L.tileOffset = r;
      launch_unpack_tiles(g0.recvSlabs[r].p, g0.fbFloat(), g0.fbRGB8(), L, tiles[r],
                          g0.stream);
    }
    HIP_CHECK(hipStreamSynchronize(g0.stream));
  }
}

}  // namespace yrt
