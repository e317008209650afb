// collectives.cpp — the sum-all-reduce behind an Engine (host callback, or RCCL over xGMI) and the life of its RCCL communicator.
#include <rccl/rccl.h>

#include <cstring>

#include "engine.hpp"
#include "pipelines.hpp"

namespace cba {

void engine_allreduce(Engine& e, double* buf, int64_t n) {
    if (n <= 0) return;
    if (e.rccl_comm) {
        if (e.coll_buf.n < static_cast<size_t>(n)) e.coll_buf.alloc(static_cast<size_t>(n) * 2);
        e.coll_pin.reserve(static_cast<size_t>(n) * 2);
        std::memcpy(e.coll_pin.p, buf, sizeof(double) * static_cast<size_t>(n));
        e.coll_buf.upload(e.coll_pin.p, static_cast<size_t>(n), e.stream);
        const ncclResult_t r = ncclAllReduce(e.coll_buf.p, e.coll_buf.p, static_cast<size_t>(n), ncclDouble, ncclSum,
                                             reinterpret_cast<ncclComm_t>(e.rccl_comm), e.stream);
        if (r != ncclSuccess) throw HipError(std::string("ncclAllReduce: ") + ncclGetErrorString(r));
        e.coll_buf.download(e.coll_pin.p, static_cast<size_t>(n), e.stream);
        CBA_HIP(hipStreamSynchronize(e.stream));
        std::memcpy(buf, e.coll_pin.p, sizeof(double) * static_cast<size_t>(n));
    } else if (e.allreduce) {
        if (e.allreduce(buf, n, e.allreduce_user) != 0) throw std::runtime_error("allreduce callback failed");
    }
}

void rccl_unique_id(uint8_t* id) {
    static_assert(sizeof(ncclUniqueId) == CBA_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    const ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) throw HipError(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(id, &u, sizeof(u));
}

void* rccl_comm_create(const uint8_t* id, int n_ranks, int rank) {
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) throw std::invalid_argument("bad rank / n_ranks");
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t comm;
    const ncclResult_t r = ncclCommInitRank(&comm, n_ranks, u, rank);
    if (r != ncclSuccess) throw HipError(std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    return comm;
}
void rccl_comm_destroy(void* comm, bool abort) {
    if (!comm) return;
    if (abort) (void)ncclCommAbort(reinterpret_cast<ncclComm_t>(comm));
    else (void)ncclCommDestroy(reinterpret_cast<ncclComm_t>(comm));
}

void rccl_init(Engine& e, const uint8_t* id, int n_ranks, int rank) {
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) throw std::invalid_argument("bad rank / n_ranks");
    rccl_destroy(e);
    e.rccl_comm = rccl_comm_create(id, n_ranks, rank);
    e.n_ranks = n_ranks;
    e.rank = rank;
}

// the abort path: this rank cannot go on (an exception in its solve, a peer that no longer answers); ncclCommAbort tears the
// communicator down without waiting for outstanding collectives, which also lets the peers' pending collectives fail instead of
// hanging (they see it through ncclCommGetAsyncError in ctl_wait, or run into their own deadline)
void rccl_abort(Engine& e) {
    if (e.rccl_comm) {
        (void)ncclCommAbort(reinterpret_cast<ncclComm_t>(e.rccl_comm));
        e.rccl_comm = nullptr;
    }
}

void rccl_destroy(Engine& e) {
    if (e.rccl_comm) {
        (void)ncclCommDestroy(reinterpret_cast<ncclComm_t>(e.rccl_comm));
        e.rccl_comm = nullptr;
    }
}

}  // namespace cba
