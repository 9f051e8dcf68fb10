// fb_comm.inc — trajectory collection over RCCL (included by fb_capi.hip inside extern "C").
// SURVEY.md §8(b) `fb_gather`, §8(e): aircraft are independent, the only exchange is ONE all-gather of the state panels over xGMI
// at collection time. RCCL is loaded lazily (dlopen) so that the library itself has no link-time dependency on it; the host
// distributes the 128-byte unique id out of band (Julia: a file or MPI; the Python mirror uses torch.distributed instead and
// never calls these).
#include <dlfcn.h>

namespace {
struct RcclApi {
    void* so = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, ncclUniqueIdBlob, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
int32_t rccl_load() {
    if (g_rccl.so) return 0;
    void* so = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!so) so = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!so) return fail("cannot load librccl.so: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void*))dlsym(so, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void**, int, ncclUniqueIdBlob, int))dlsym(so, "ncclCommInitRank");
    g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(so, "ncclAllGather");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(so, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(so, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy) return fail("librccl.so lacks an expected symbol");
    g_rccl.so = so;
    return 0;
}
int32_t rccl_check(int rc, const char* what) {
    if (rc == 0) return 0;
    return fail("%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
}
}  // namespace

// What fb_comm_init hands back: the RCCL communicator plus every rank's shard size, exchanged once at init time (one 8-byte
// all-gather) so that fb_gather_state can deal with ragged shards instead of mis-gathering them silently.
struct FbComm {
    void* nccl = nullptr;
    int32_t world = 0, rank = 0;
    std::vector<int64_t> n_of;   // [world]
    int64_t n_max = 0;
    bool ragged = false;
    double* stage = nullptr;     // ragged shards only: this rank's rows padded to n_max, [Nx x n_max]
    int device = 0;
};

extern "C" {
int32_t fb_comm_unique_id(char* id128) {
    if (!id128) return fail("null argument");
    if (int32_t rc = rccl_load()) return rc;
    return rccl_check(g_rccl.GetUniqueId(id128), "ncclGetUniqueId");
}
int32_t fb_comm_destroy(void* comm);
int32_t fb_comm_init(fb_handle h, int32_t world, int32_t rank, const char* id128, void** comm) {
    if (!h || !id128 || !comm) return fail("null argument");
    if (is_lss(h)) return lss_refuse("fb_comm_init", "gathering LinearizedSS states over RCCL is not implemented");
    if (world < 1 || rank < 0 || rank >= world) return fail("fb_comm_init: rank %d of %d", rank, world);
    if (int32_t rc = rccl_load()) return rc;
    HIPCHK(hipSetDevice(h->device));   // one communicator per rank, on the handle's GPU
    ncclUniqueIdBlob id;
    std::memcpy(id.internal, id128, sizeof id.internal);
    FbComm* c = new FbComm();
    c->world = world; c->rank = rank; c->device = h->device;
    if (int32_t rc = rccl_check(g_rccl.CommInitRank(&c->nccl, world, id, rank), "ncclCommInitRank")) { delete c; return rc; }
    // shard sizes of all ranks (collective)
    int64_t* d = nullptr;
    auto bail = [&](int32_t rc) { if (d) (void)hipFree(d); (void)fb_comm_destroy(c); return rc; };
    if (hipMalloc(&d, sizeof(int64_t) * (world + 1)) != hipSuccess) return bail(fail("fb_comm_init: hipMalloc failed"));
    const int64_t mine = h->n;
    if (hipMemcpyAsync(d + world, &mine, sizeof mine, hipMemcpyHostToDevice, h->stream) != hipSuccess) return bail(fail("fb_comm_init: copy failed"));
    if (int32_t rc = rccl_check(g_rccl.AllGather(d + world, d, 1, 4 /* ncclInt64 */, c->nccl, h->stream), "ncclAllGather(shard sizes)")) return bail(rc);
    c->n_of.resize(world);
    if (hipMemcpyAsync(c->n_of.data(), d, sizeof(int64_t) * world, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail("fb_comm_init: reading the shard sizes back failed"));
    (void)hipFree(d); d = nullptr;
    for (int r = 0; r < world; r++) { if (c->n_of[r] > c->n_max) c->n_max = c->n_of[r]; if (c->n_of[r] != c->n_of[0]) c->ragged = true; }
    if (c->n_of[rank] != h->n) return bail(fail("fb_comm_init: shard size exchange returned %lld for this rank, the handle holds %lld", (long long)c->n_of[rank], (long long)h->n));
    *comm = c;
    return 0;
}
int32_t fb_comm_destroy(void* comm) {
    if (!comm) return 0;
    FbComm* c = (FbComm*)comm;
    int32_t rc = 0;
    if (c->nccl) { if ((rc = rccl_load()) == 0) rc = rccl_check(g_rccl.CommDestroy(c->nccl), "ncclCommDestroy"); }
    if (c->stage) { (void)hipSetDevice(c->device); (void)hipFree(c->stage); }
    delete c;
    return rc;
}
int32_t fb_comm_shard_sizes(void* comm, int64_t* n_of, int64_t* n_max) {
    if (!comm) return fail("null argument");
    FbComm* c = (FbComm*)comm;
    if (n_of) for (int r = 0; r < c->world; r++) n_of[r] = c->n_of[r];
    if (n_max) *n_max = c->n_max;
    return 0;
}
int32_t fb_gather_state(fb_handle h, void* comm, double* recv_dev) {
    if (!h || !comm || !recv_dev) return fail("null argument");
    if (h->model == FB_MODEL_ROBOT2D) return fail("fb_gather_state: not available for Robot2D handles");
    if (is_lss(h)) return lss_refuse("fb_gather_state", "gathering LinearizedSS states over RCCL is not implemented");
    if (int32_t rc = rccl_load()) return rc;
    FbComm* c = (FbComm*)comm;
    if (c->n_of[c->rank] != h->n) return fail("fb_gather_state: the communicator was initialised with a handle of %lld aircraft, this one holds %lld", (long long)c->n_of[c->rank], (long long)h->n);
    HIPCHK(hipSetDevice(h->device));
    const size_t nx = (size_t)(is_x2(h) ? (int)FB_X2_NX : (int)FB_NX);   // device rows
    const double* send = h->x;
    if (c->ragged) {
        // an all-gather moves the same count from every rank: pad this rank's rows to n_max (the tail of a row is left as it is; the
        // receiver reads n_of[r] entries per row, fb_comm_shard_sizes)
        if (!c->stage) HIPCHK(hipMalloc(&c->stage, sizeof(double) * nx * (size_t)c->n_max));
        HIPCHK(hipMemcpy2DAsync(c->stage, sizeof(double) * (size_t)c->n_max, h->x, sizeof(double) * (size_t)h->n, sizeof(double) * (size_t)h->n, nx,
                                hipMemcpyDeviceToDevice, h->stream));
        send = c->stage;
    }
    return rccl_check(g_rccl.AllGather(send, recv_dev, nx * (size_t)c->n_max, 8 /* ncclFloat64 */, c->nccl, h->stream), "ncclAllGather");
}
}  // extern "C"
