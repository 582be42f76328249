// The path's one exchange step behind the C-ABI: an all-gather of every rank's orientation bitsets over RCCL, enqueued on the
// context's stream (SURVEY.md section 8e; it stands in for the reference's gather-to-root + broadcast of the winner's BitSets,
// main.cpp:1421-1601, mpi_util.cpp:152-233).  A C++ host needs neither torch nor a host hop per collective: rank 0 calls
// pcr_comm_unique_id, ships the 128 bytes to the other ranks however it likes (the reference has MPI_Bcast for that, main.cpp:99),
// every rank calls pcr_comm_init_rank once, then pcr_exchange_bits per pass.
//
// RCCL is bound at run time (dlopen), not at link time: the library that is ALREADY in the process is taken first -- a process
// that runs PyTorch has torch's own librccl + libamdhip64 loaded, and a second RCCL on a second HIP runtime must not join it
// (INTEGRATION.md section 4) -- then librccl.so.1 from the loader's path, then /opt/rocm/lib.  PCRAMP_RCCL=<path> overrides.
#include <dlfcn.h>
#include <rccl/rccl.h>       // types and enumerators only: no RCCL symbol is referenced at link time

struct pcr_comm {
	ncclComm_t comm = nullptr;   // RCCL communicator (pcr_comm_init_rank); nullptr for a host-collective one
	pcr_host_allgather_fn host_fn = nullptr; void *host_user = nullptr;   // the caller's all-gather (pcr_comm_init_host)
	int world = 0, rank = 0;
	int device = 0;              // the communicator belongs to this device: any handle on it may exchange through it
};

namespace {

struct RcclApi {
	void *handle = nullptr;
	ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
	ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
	ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	const char *(*GetErrorString)(ncclResult_t) = nullptr;
	std::string path;
};

RcclApi *rccl_api()
{
	static RcclApi api;
	static bool tried = false;
	if(tried) return api.handle ? &api : nullptr;
	tried = true;
	std::vector<std::pair<std::string, int> > cand;
	if(const char *v = getenv("PCRAMP_RCCL")) cand.push_back(std::make_pair(std::string(v), RTLD_NOW | RTLD_GLOBAL));
	for(const char *n : {"librccl.so", "librccl.so.1"}) cand.push_back(std::make_pair(std::string(n), RTLD_NOW | RTLD_NOLOAD));   // already in the process
	for(const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) cand.push_back(std::make_pair(std::string(n), RTLD_NOW | RTLD_GLOBAL));
	for(const auto &c : cand){
		void *h = dlopen(c.first.c_str(), c.second);
		if(!h) continue;
		RcclApi a;
		a.handle = h; a.path = c.first;
		a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
		a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
		a.AllGather = (decltype(a.AllGather))dlsym(h, "ncclAllGather");
		a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
		a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
		if(a.GetUniqueId && a.CommInitRank && a.AllGather && a.CommDestroy && a.GetErrorString){ api = a; return &api; }
		dlclose(h);
	}
	g_err = "RCCL not found (librccl.so.1 is neither loaded nor on the library path; set PCRAMP_RCCL)";
	return nullptr;
}

#define RCCL_TRY(api, expr) do{ const ncclResult_t r_ = (expr); if(r_ != ncclSuccess){ \
	g_err = std::string(#expr) + ": " + (api)->GetErrorString(r_); return PCR_ERR_DEVICE; } }while(0)

} // namespace

extern "C" {

int pcr_comm_unique_id(uint8_t id[PCR_COMM_ID_BYTES])
{
	static_assert(PCR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the ABI's id is RCCL's ncclUniqueId");
	if(!id){ g_err = "pcr_comm_unique_id: null id"; return PCR_ERR_ARG; }
	RcclApi *api = rccl_api();
	if(!api) return PCR_ERR_STATE;
	ncclUniqueId u;
	RCCL_TRY(api, api->GetUniqueId(&u));
	memcpy(id, u.internal, PCR_COMM_ID_BYTES);
	return PCR_OK;
}

pcr_comm *pcr_comm_init_rank(pcr_ctx *ctx, const uint8_t id[PCR_COMM_ID_BYTES], int world, int rank)
{
	if(!ctx || !id || world < 1 || rank < 0 || rank >= world){ g_err = "pcr_comm_init_rank: bad argument"; return nullptr; }
	RcclApi *api = rccl_api();
	if(!api) return nullptr;
	if(hipSetDevice(ctx->device) != hipSuccess){ g_err = "pcr_comm_init_rank: hipSetDevice failed"; return nullptr; }
	ncclUniqueId u;
	memcpy(u.internal, id, PCR_COMM_ID_BYTES);
	pcr_comm *c = new pcr_comm();
	c->world = world; c->rank = rank; c->device = ctx->device;
	const ncclResult_t r = api->CommInitRank(&c->comm, world, u, rank);
	if(r != ncclSuccess){ g_err = std::string("ncclCommInitRank: ") + api->GetErrorString(r); delete c; return nullptr; }
	return c;
}

pcr_comm *pcr_comm_init_host(pcr_ctx *ctx, int world, int rank, pcr_host_allgather_fn fn, void *user)
{
	if(!ctx || !fn || world < 1 || rank < 0 || rank >= world){ g_err = "pcr_comm_init_host: bad argument"; return nullptr; }
	pcr_comm *c = new pcr_comm();
	c->host_fn = fn; c->host_user = user;
	c->world = world; c->rank = rank; c->device = ctx->device;
	return c;
}

int pcr_comm_world(const pcr_comm *comm) { return comm ? comm->world : 0; }
int pcr_comm_rank(const pcr_comm *comm) { return comm ? comm->rank : -1; }

int pcr_exchange_bits(pcr_ctx *ctx, pcr_comm *comm, const uint64_t *d_local, uint64_t words_per_rank, uint64_t *d_full)
{
	if(!ctx || !comm || comm->device != ctx->device || (words_per_rank && (!d_local || !d_full))){ g_err = "pcr_exchange_bits: bad argument (the communicator belongs to another device?)"; return PCR_ERR_ARG; }
	if(comm->host_fn){                                                            // host collective: device -> host, the caller's all-gather, host -> device
		DRAIN(ctx);
		HIP_TRY(hipSetDevice(ctx->device));
		if(words_per_rank == 0) return PCR_OK;
		std::vector<uint64_t> send(words_per_rank), recv((size_t)words_per_rank*comm->world);
		HIP_TRY(hipMemcpyAsync(send.data(), d_local, words_per_rank*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		if(comm->host_fn(send.data(), words_per_rank*sizeof(uint64_t), recv.data(), comm->host_user) != 0){ g_err = "pcr_exchange_bits: the host all-gather failed"; return PCR_ERR_DEVICE; }
		HIP_TRY(hipMemcpyAsync(d_full, recv.data(), recv.size()*sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));                               // (recv is about to go away)
		return PCR_OK;
	}
	RcclApi *api = rccl_api();
	if(!api) return PCR_ERR_STATE;
	// a pass enqueued by pcr_screen_device has final bitsets only once its counters have been looked at (a bucket overflow replays
	// it into the same buffers): never let the collective read a buffer a replay could still rewrite
	DRAIN(ctx);
	HIP_TRY(hipSetDevice(ctx->device));
	if(words_per_rank == 0) return PCR_OK;
	RCCL_TRY(api, api->AllGather(d_local, d_full, (size_t)words_per_rank, ncclUint64, comm->comm, ctx->stream));
	return PCR_OK;
}

void pcr_comm_destroy(pcr_comm *comm)
{
	if(!comm) return;
	RcclApi *api = comm->comm ? rccl_api() : nullptr;
	if(api && comm->comm){
		(void)hipSetDevice(comm->device); (void)hipDeviceSynchronize();
		(void)api->CommDestroy(comm->comm);
	}
	delete comm;
}

const char *pcr_comm_library(void)
{
	RcclApi *api = rccl_api();
	return api ? api->path.c_str() : "";
}

} // extern "C"
