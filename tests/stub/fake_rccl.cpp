// fake_rccl.cpp -- TEST INFRASTRUCTURE ONLY: a stand-in for the eight RCCL entry points pt_comm.cpp resolves (csrc/pt_comm.cpp, load_rccl),
// so that the library's N-rank plumbing - unique id, ncclCommInitRank per process, ONE reduce per frame and rank whatever buffers the
// caller passed, RGBA8 pack on the root, communicator reuse and teardown - runs with N > 1 processes on a box that has ONE GPU
// (tests/test_multi_rank_gpu.py::test_library_reduce_with_stub_collective; selected with PT_RCCL_PATH).  It is not RCCL and proves
// nothing about RCCL: ranks meet in a directory under /tmp named by the unique id, a reduce is a blocking sum through files.  The real
// library is exercised by the same test on boxes with N GPUs (test_library_reduce_across_processes) and by bench.py --gpus N.
//
// Second mode, one process / N ranks (ncclCommInitAll; tests/test_group_gpu.py, `pt_main --devices 0,0`): the n communicators share
// one in-process record.  DUPLICATE DEVICES ARE ALLOWED - the real RCCL refuses them; running N ranks on one card is the point of
// this stub, and again: this is not RCCL and proves nothing about RCCL.  An ncclReduce on such a communicator is only recorded inside
// ncclGroupStart / ncclGroupEnd (per-thread nesting count) and executed by the outermost ncclGroupEnd; outside a group it returns
// ncclInvalidUsage, because one host thread cannot complete a blocking N-rank reduce rank by rank (the real library would hang).
// The execution is strict where the real library would hang or corrupt: every rank of the communicator exactly once, with the same
// count, datatype, op and root, else ncclInvalidUsage.  The sum is formed on the host in the order of the process mode (the root's
// buffer, then the others by rank), so both modes are comparable bit for bit; every NON-root receive buffer is filled with quiet NaNs
// (NCCL leaves it unspecified: a caller that reads one must show up as NaNs in a frame, not pass by luck).
//
// FAKE_RCCL_FAIL (read at call time) makes one entry point return ncclInternalError ON THE HOST, without touching the GPU:
// "initall" -> ncclCommInitAll, "reduce:<rank>" -> ncclReduce of that rank, "groupend" -> the outermost ncclGroupEnd (which then
// drops the recorded calls).  It injects a return code only: no GPU work is launched, cut short or corrupted by it.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

struct InProcess { // one per ncclCommInitAll, shared by its communicators
    std::vector<int> device; // of every rank
};

struct ncclComm {
    int rank, world;
    std::string dir;
    unsigned long seq;
    std::shared_ptr<InProcess> shared; // null: the process-per-rank mode
};

namespace {
bool wait_for(const std::string& path, double seconds)
{
    const auto t0 = std::chrono::steady_clock::now();
    struct stat st;
    while (stat(path.c_str(), &st) != 0) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
    return true;
}
bool write_file(const std::string& path, const void* data, size_t bytes)
{
    const std::string tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, bytes, f) == bytes;
    fclose(f);
    return ok && rename(tmp.c_str(), path.c_str()) == 0;
}

struct Pending { // an ncclReduce recorded inside a group
    ncclComm* comm;
    const void* send;
    void* recv;
    size_t count;
    ncclDataType_t datatype;
    ncclRedOp_t op;
    int root;
    hipStream_t stream;
};
thread_local int t_group_depth = 0;
thread_local std::vector<Pending> t_pending;

bool inject(const std::string& what)
{
    const char* e = getenv("FAKE_RCCL_FAIL");
    return e && what == e;
}

// the recorded reduces of ONE in-process communicator set, one per rank; the calls may be in place, so every buffer is read before
// the first one is written
ncclResult_t run_reduce(const InProcess& s, const std::vector<const Pending*>& by_rank)
{
    const int world = (int)s.device.size();
    const int root = by_rank[0]->root;
    const size_t n = by_rank[0]->count;
    std::vector<std::vector<float>> data((size_t)world, std::vector<float>(n));
    for (int r = 0; r < world; ++r) {
        const Pending& p = *by_rank[(size_t)r];
        if (hipSetDevice(s.device[(size_t)r]) != hipSuccess || hipStreamSynchronize(p.stream) != hipSuccess ||
            hipMemcpy(data[(size_t)r].data(), p.send, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return ncclUnhandledCudaError;
    }
    std::vector<float>& sum = data[(size_t)root];
    for (int r = 0; r < world; ++r) {
        if (r == root) continue;
        for (size_t i = 0; i < n; ++i) sum[i] += data[(size_t)r][i];
    }
    const std::vector<uint32_t> nan(n, 0x7fc00000u);
    for (int r = 0; r < world; ++r) {
        const void* src = r == root ? (const void*)sum.data() : (const void*)nan.data();
        if (hipSetDevice(s.device[(size_t)r]) != hipSuccess || hipMemcpy(by_rank[(size_t)r]->recv, src, n * 4, hipMemcpyHostToDevice) != hipSuccess)
            return ncclUnhandledCudaError;
    }
    return ncclSuccess;
}

ncclResult_t run_pending(const std::vector<Pending>& calls)
{
    std::vector<char> seen(calls.size(), 0);
    for (size_t i = 0; i < calls.size(); ++i) {
        if (seen[i]) continue;
        const InProcess* s = calls[i].comm->shared.get();
        std::vector<const Pending*> by_rank(s->device.size(), nullptr);
        for (size_t j = i; j < calls.size(); ++j) {
            if (calls[j].comm->shared.get() != s) continue;
            seen[j] = 1;
            const Pending*& slot = by_rank[(size_t)calls[j].comm->rank];
            if (slot) return ncclInvalidUsage; // a rank twice in one group
            slot = &calls[j];
        }
        for (const Pending* p : by_rank) {
            if (!p) return ncclInvalidUsage; // a rank is missing: the real reduce would never complete
            const Pending& a = *by_rank[0];
            if (p->count != a.count || p->datatype != a.datatype || p->op != a.op || p->root != a.root) return ncclInvalidUsage;
        }
        const ncclResult_t r = run_reduce(*s, by_rank);
        if (r != ncclSuccess) return r;
    }
    return ncclSuccess;
}
} // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* id)
{
    std::memset(id->internal, 0, sizeof(id->internal));
    snprintf(id->internal, sizeof(id->internal), "fake_rccl_%d_%lld", (int)getpid(), (long long)std::chrono::steady_clock::now().time_since_epoch().count());
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank)
{
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    ncclComm* c = new ncclComm{rank, nranks, std::string("/tmp/") + std::string(id.internal, strnlen(id.internal, sizeof(id.internal))), 0, nullptr};
    mkdir(c->dir.c_str(), 0700); // every rank may be first
    const char one = 1;
    if (!write_file(c->dir + "/init_" + std::to_string(rank), &one, 1)) { delete c; return ncclSystemError; }
    for (int r = 0; r < nranks; ++r)
        if (!wait_for(c->dir + "/init_" + std::to_string(r), 120.0)) { delete c; return ncclSystemError; }
    *comm = c;
    return ncclSuccess;
}

ncclResult_t ncclCommInitAll(ncclComm_t* comms, int n, const int* devs)
{
    if (inject("initall")) return ncclInternalError;
    if (!comms || n < 1) return ncclInvalidArgument;
    auto s = std::make_shared<InProcess>();
    for (int r = 0; r < n; ++r) {
        const int d = devs ? devs[r] : r; // NULL: 0..n-1 as in NCCL
        if (d < 0) return ncclInvalidArgument;
        s->device.push_back(d); // duplicates allowed (see the file comment)
    }
    for (int r = 0; r < n; ++r) comms[r] = new ncclComm{r, n, std::string(), 0, s};
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    delete comm;
    return ncclSuccess;
}

// process mode - blocking: drains `stream`, then non-roots publish their buffer, the root adds them to its own in rank order;
// in-process mode: recorded for ncclGroupEnd
ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, int root, ncclComm_t comm, hipStream_t stream)
{
    if (!comm || datatype != ncclFloat32 || op != ncclSum || root < 0 || root >= comm->world) return ncclInvalidArgument;
    if (inject("reduce:" + std::to_string(comm->rank))) return ncclInternalError;
    if (comm->shared) {
        if (t_group_depth == 0) return ncclInvalidUsage;
        t_pending.push_back({comm, sendbuff, recvbuff, count, datatype, op, root, stream});
        return ncclSuccess;
    }
    if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;
    const unsigned long seq = comm->seq++;
    std::vector<float> mine(count);
    if (hipMemcpy(mine.data(), sendbuff, count * 4, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
    const std::string base = comm->dir + "/red_" + std::to_string(seq) + "_";
    if (comm->rank != root) {
        if (!write_file(base + std::to_string(comm->rank), mine.data(), count * 4)) return ncclSystemError;
        // (like the real call, a non-root may return before the root is done; its receive buffer is unspecified)
        return ncclSuccess;
    }
    std::vector<float> other(count);
    for (int r = 0; r < comm->world; ++r) {
        if (r == root) continue;
        const std::string path = base + std::to_string(r);
        if (!wait_for(path, 300.0)) return ncclSystemError;
        FILE* f = fopen(path.c_str(), "rb");
        if (!f || fread(other.data(), 1, count * 4, f) != count * 4) { if (f) fclose(f); return ncclSystemError; }
        fclose(f);
        remove(path.c_str());
        for (size_t i = 0; i < count; ++i) mine[i] += other[i];
    }
    if (hipMemcpy(recvbuff, mine.data(), count * 4, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
    return ncclSuccess;
}

ncclResult_t ncclGroupStart()
{
    ++t_group_depth;
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd()
{
    if (t_group_depth == 0) return ncclInvalidUsage;
    if (--t_group_depth > 0) return ncclSuccess;
    std::vector<Pending> calls;
    calls.swap(t_pending); // whatever happens below, the next group starts empty
    if (inject("groupend")) return ncclInternalError;
    if (calls.empty()) return ncclSuccess;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ncclUnhandledCudaError;
    const ncclResult_t r = run_pending(calls);
    if (hipSetDevice(dev) != hipSuccess) return ncclUnhandledCudaError; // the caller's current device, as the real library leaves it
    return r;
}

const char* ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error (fake_rccl)";
    case ncclInvalidUsage: return "invalid usage (fake_rccl)";
    case ncclInternalError: return "internal error (fake_rccl)";
    default: return "fake_rccl error";
    }
}

} // extern "C"
