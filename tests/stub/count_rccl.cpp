// count_rccl.cpp -- TEST INFRASTRUCTURE ONLY: a forwarding shim in front of whatever PT_RCCL_PATH would otherwise name (the stub collective
// of fake_rccl.cpp, or a real RCCL): it resolves the eight entry points pt_comm.cpp uses from the library in COUNT_RCCL_TARGET, passes
// every call on unchanged and counts the ncclReduce calls of this process (count_rccl_reduces), so that a test can state "ONE reduce
// per launch sequence and rank" as a number (tests/test_gpu_batch.py::test_batch_reduce_with_stub_collective).  It adds nothing to
// a collective and touches no GPU.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cstdlib>

namespace {
std::atomic<int> g_reduces{0};
void* target()
{
    static void* h = [] {
        const char* p = getenv("COUNT_RCCL_TARGET");
        return p && p[0] ? dlopen(p, RTLD_NOW | RTLD_LOCAL) : nullptr;
    }();
    return h;
}
template <typename F>
F sym(const char* name)
{
    void* h = target();
    return h ? reinterpret_cast<F>(dlsym(h, name)) : nullptr;
}
} // namespace

extern "C" {
int count_rccl_reduces(void) { return g_reduces.load(); }

ncclResult_t ncclGetUniqueId(ncclUniqueId* id)
{
    auto f = sym<decltype(&ncclGetUniqueId)>("ncclGetUniqueId");
    return f ? f(id) : ncclSystemError;
}
ncclResult_t ncclCommInitRank(ncclComm_t* comm, int n, ncclUniqueId id, int rank)
{
    auto f = sym<decltype(&ncclCommInitRank)>("ncclCommInitRank");
    return f ? f(comm, n, id, rank) : ncclSystemError;
}
ncclResult_t ncclCommInitAll(ncclComm_t* comms, int n, const int* devs)
{
    auto f = sym<decltype(&ncclCommInitAll)>("ncclCommInitAll");
    return f ? f(comms, n, devs) : ncclSystemError;
}
ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    auto f = sym<decltype(&ncclCommDestroy)>("ncclCommDestroy");
    return f ? f(comm) : ncclSystemError;
}
ncclResult_t ncclReduce(const void* send, void* recv, size_t count, ncclDataType_t type, ncclRedOp_t op, int root, ncclComm_t comm, hipStream_t stream)
{
    auto f = sym<decltype(&ncclReduce)>("ncclReduce");
    if (!f) return ncclSystemError;
    ++g_reduces;
    return f(send, recv, count, type, op, root, comm, stream);
}
ncclResult_t ncclGroupStart()
{
    auto f = sym<decltype(&ncclGroupStart)>("ncclGroupStart");
    return f ? f() : ncclSystemError;
}
ncclResult_t ncclGroupEnd()
{
    auto f = sym<decltype(&ncclGroupEnd)>("ncclGroupEnd");
    return f ? f() : ncclSystemError;
}
const char* ncclGetErrorString(ncclResult_t r)
{
    auto f = sym<decltype(&ncclGetErrorString)>("ncclGetErrorString");
    return f ? f(r) : "count_rccl: COUNT_RCCL_TARGET could not be loaded";
}
}
