// The C ABI of libzkgpu_stark (include/zkgpu_stark.h): the prover's entry
// points, the transcript's and the communicators'.
#include "comm_host.hpp"
#include "comm_rccl.hpp"
#include "sharded_starks.hpp"

using namespace zkgpu_host;

static Starks &prover(void *h) { return *(Starks *)h; }
// The entry points of the single-GPU prover only (its diagnostics, the
// streamed stage 1, the .exec hand-off): a row-sharded handle is refused
// here, before the call looks at its arguments, for the reason `why` gives
// (true: fail() has set the text; its -1 is the `true`).
static bool refused(void *h, const char *why) { return prover(h).sharded && fail("stark (sharded): %s", why); }

extern "C" {

const char *zkgpu_stark_last_error(void) { return zkgpu_host::g_err; }

int zkgpu_stark_create_ex(void **handle, const zkgpu_stark_info *info, uint32_t memory_plan)
{
    Starks *s = new Starks();
    if (s->create(info, memory_plan)) {
        delete s;
        *handle = nullptr;
        return -1;
    }
    *handle = s;
    return 0;
}

int zkgpu_stark_create(void **handle, const zkgpu_stark_info *info)
{
    return zkgpu_stark_create_ex(handle, info, ZKGPU_MEM_AUTO);
}

int zkgpu_stark_memory_mode(void *h) { return prover(h).mem_mode; }

int zkgpu_stark_witness(void *h) { return prover(h).witness(); }
int zkgpu_stark_set_cm1(void *h, const uint64_t *rows) { return prover(h).set_cm1(rows); }
int zkgpu_stark_set_cm1_async(void *h, const uint64_t *rows) { return prover(h).set_cm1_async(rows); }
int zkgpu_stark_get_cm1(void *h, uint64_t *rows)
{
    return refused(h, "get_cm1 is single-GPU only") ? -1 : prover(h).get_cm1(rows);
}
int zkgpu_stark_set_exec(void *h, const uint64_t *image, uint64_t image_words, uint64_t size_witness)
{
    if (refused(h, "set_exec is single-GPU only (the recursion circuits' traces fit one device)")) return -1;
    return prover(h).set_exec(image, image_words, size_witness);
}
int zkgpu_stark_set_cm1_witness(void *h, const uint64_t *witness)
{
    if (refused(h, "set_cm1_witness is single-GPU only (the recursion circuits' traces fit one device)")) return -1;
    return prover(h).set_cm1_witness(witness);
}
int zkgpu_stark_set_const(void *h, const uint64_t *rows) { return prover(h).set_const(rows); }
int zkgpu_stark_set_publics(void *h, const uint64_t *publics) { return prover(h).set_publics(publics); }
uint64_t zkgpu_stark_proof_len(void *h) { return prover(h).proof_len(); }
int zkgpu_stark_prove(void *h, uint64_t *out) { return prover(h).prove(out); }
int zkgpu_stark_prove_from_rows(void *h, const uint64_t *rows, int register_host, uint64_t *out)
{
    if (refused(h, "prove_from_rows is single-GPU only (each rank loads its rows: set_cm1 / set_cm1_async, then "
                   "prove)"))
        return -1;
    return prover(h).prove_from_rows(rows, register_host, out);
}
int zkgpu_stark_verkey(void *h, uint64_t out[4])
{
    memcpy(out, prover(h).verkey, 32);
    return 0;
}
int zkgpu_stark_publics(void *h, uint64_t *out)
{
    const std::vector<uint64_t> &p = prover(h).publics;
    memcpy(out, p.data(), p.size() * 8);
    return (int)p.size();
}
int zkgpu_stark_timers(void *h, char *names_buf, uint64_t names_len, double *ms, uint32_t max)
{
    std::string names;
    uint32_t n = 0;
    for (auto &t : prover(h).timers) {
        if (n >= max) break;
        names += t.first + "\n";
        ms[n++] = t.second;
    }
    if (names_len) {
        size_t c = names.size() < names_len - 1 ? names.size() : names_len - 1;
        memcpy(names_buf, names.data(), c);
        names_buf[c] = 0;
    }
    return (int)n;
}
void zkgpu_stark_destroy(void *h) { delete (Starks *)h; }

// ---- the diagnostics (starks.hpp Probe, Checks).  The readers of a result
// are not refused: a row-sharded prover never ran a diagnostic, and says so.
int zkgpu_stark_probe_set(void *h, const uint64_t *rows_n, uint32_t n_rows_n, const uint64_t *rows_ext,
                          uint32_t n_rows_ext)
{
    if (refused(h, "probe_set is single-GPU only (the sampled rows live on other ranks)")) return -1;
    return prover(h).probe.set(prover(h), rows_n, n_rows_n, rows_ext, n_rows_ext);
}
int zkgpu_stark_probe_size(void *h, uint32_t *n_recs, uint64_t *n_words)
{
    return prover(h).probe.size(n_recs, n_words);
}
int zkgpu_stark_probe_read(void *h, zkgpu_probe_rec *recs, uint32_t max_recs, uint64_t *payload, uint64_t max_words)
{
    return prover(h).probe.read(recs, max_recs, payload, max_words);
}
int zkgpu_stark_check_set(void *h, uint32_t mode)
{
    if (refused(h, "check_set is single-GPU only (the n-domain sections live in row blocks on the ranks)")) return -1;
    return prover(h).checks.set(prover(h), mode);
}
int zkgpu_stark_check_result(void *h, zkgpu_check_result *out) { return prover(h).checks.result(out); }
int zkgpu_stark_check_names_set(void *h, int on)
{
    if (refused(h, "check_names_set is single-GPU only (as check_set)")) return -1;
    return prover(h).checks.names_set(prover(h), on);
}
int zkgpu_stark_check_terms(void *h, zxp_split_term *out, uint32_t max, uint32_t *n)
{
    return prover(h).checks.terms(out, max, n);
}
int zkgpu_stark_check_named(void *h, uint32_t slot, uint32_t *ids, uint64_t *values, uint32_t max, uint32_t *n_failing)
{
    return prover(h).checks.named(slot, ids, values, max, n_failing);
}
int zkgpu_stark_z_diag(void *h, zkgpu_z_diag *out)
{
    if (refused(h, "z_diag: single-GPU provers only (a rank holds a row block of num and den)")) return -1;
    return prover(h).checks.z_diag(out);
}
int zkgpu_stark_audit(void *h, uint32_t flags, zkgpu_audit_report *out)
{
    if (refused(h, "audit: single-GPU provers only (a rank holds a row block of the n-domain sections)")) return -1;
    return prover(h).checks.audit(prover(h), flags, out);
}
int zkgpu_stark_audit_format(void *h, char *buf, uint64_t len)
{
    if (refused(h, "audit_format: single-GPU provers only")) return -1;
    return prover(h).checks.audit_format(prover(h), buf, len);
}
int zkgpu_stark_conn_set(void *h, uint32_t z, const zkgpu_conn_desc *d)
{
    if (refused(h, "conn_set: single-GPU provers only (as the audit)")) return -1;
    return prover(h).checks.conn_set(prover(h), z, d);
}
int zkgpu_stark_conn_check(void *h, uint32_t z, zkgpu_conn_report *out)
{
    if (refused(h, "conn_check: single-GPU provers only (a rank holds a row block of the n-domain sections)"))
        return -1;
    return prover(h).checks.conn_check(prover(h), z, out);
}
int zkgpu_stark_audit_conn(void *h, uint32_t k, zkgpu_conn_report *out)
{
    return refused(h, "audit_conn: single-GPU provers only") ? -1 : prover(h).checks.audit_conn(k, out);
}

// ---- the prover's own Transcript class behind the reference's Transcript surface
struct zkgpu_transcript {
    zkgpu_host::Transcript t;
};
zkgpu_transcript *zkgpu_transcript_create(void) { return new zkgpu_transcript(); }
void zkgpu_transcript_destroy(zkgpu_transcript *t) { delete t; }
int zkgpu_transcript_put(zkgpu_transcript *t, const uint64_t *in, uint64_t n)
{
    if (!t || (n && !in)) return fail("transcript_put: null argument");
    t->t.put(in, n);
    return t->t.err ? fail("transcript_put: host permutation failed") : 0;
}
int zkgpu_transcript_get_fields1(zkgpu_transcript *t, uint64_t *out)
{
    if (!t || !out) return fail("transcript_get_fields1: null argument");
    *out = t->t.get_fields1();
    return t->t.err ? fail("transcript_get_fields1: host permutation failed") : 0;
}
int zkgpu_transcript_get_field(zkgpu_transcript *t, uint64_t out[3])
{
    if (!t || !out) return fail("transcript_get_field: null argument");
    t->t.get_field(out);
    return t->t.err ? fail("transcript_get_field: host permutation failed") : 0;
}
int zkgpu_transcript_get_permutations(zkgpu_transcript *t, uint64_t *res, uint64_t n, uint64_t nbits)
{
    if (!t || (n && !res)) return fail("transcript_get_permutations: null argument");
    if (nbits == 0 || nbits > 63) return fail("transcript_get_permutations: nbits %lu not in [1, 63]", (unsigned long)nbits);
    if (n == 0) return 0;
    t->t.get_permutations(res, n, nbits);
    return t->t.err ? fail("transcript_get_permutations: host permutation failed") : 0;
}

// ---- the row-sharded prover and the memory plans
int zkgpu_stark_create_sharded(void **handle, const zkgpu_stark_info *info, const zkgpu_comm *comm)
{
    *handle = nullptr;
    if (!comm) return fail("stark_create_sharded: no communicator");
    ShardedStarks *s = new ShardedStarks();
    if (s->create_sharded(info, comm)) {
        delete s;
        return -1;
    }
    *handle = s;
    return 0;
}

int zkgpu_stark_memory_plan(const zkgpu_stark_info *info, uint32_t world, uint64_t *bytes_per_gpu)
{
    if (!info || !bytes_per_gpu) return fail("stark_memory_plan: null argument");
    *bytes_per_gpu = 0;
    if (world) {
        ShardedStarks s;
        return s.shape(info, world, 0, false) ? -1 : s.plan(bytes_per_gpu);
    }
    Starks s;
    return s.load(info, false) ? -1 : s.plan(bytes_per_gpu);
}

int zkgpu_stark_memory_plan_ex(const zkgpu_stark_info *info, uint32_t memory_plan, uint64_t *bytes)
{
    if (!info || !bytes) return fail("stark_memory_plan_ex: null argument");
    *bytes = 0;
    if (memory_plan > ZKGPU_MEM_LEAN) return fail("stark_memory_plan_ex: unknown plan %u", memory_plan);
    Starks s;
    if (s.load(info, false)) return -1;
    if (memory_plan == ZKGPU_MEM_LEAN) {
        std::string why;
        if (!s.lean_ok(why)) return fail("stark_memory_plan_ex: the lean plan does not apply: %s", why.c_str());
        s.set_mode(ZKGPU_MEM_LEAN, false);  // (no device: no kept columns)
    }
    return s.plan(bytes);
}

// ---- the communicators (comm_rccl.hpp, comm_host.hpp)
int zkgpu_comm_rccl_unique_id(uint8_t id[128])
{
    using zkgpu_host::g_rccl;
    if (g_rccl.load()) return -1;
    ncclUniqueId u;
    ncclResult_t r = g_rccl.get_unique_id(&u);
    if (r != ncclSuccess) return fail("ncclGetUniqueId: %s", g_rccl.error_string(r));
    static_assert(sizeof u == 128, "ncclUniqueId size");
    memcpy(id, &u, 128);
    return 0;
}

int zkgpu_comm_rccl_create(zkgpu_comm *comm, const uint8_t id[128], uint32_t world, uint32_t rank)
{
    using zkgpu_host::g_rccl;
    memset(comm, 0, sizeof *comm);
    if (g_rccl.load()) return -1;
    if (zkgpu_init(-1)) return fail("zkgpu_comm_rccl_create: %s", zkgpu_last_error());
    ncclUniqueId u;
    memcpy(&u, id, 128);
    auto *ctx = new zkgpu_host::RcclCtx();
    ncclResult_t r = g_rccl.comm_init_rank(&ctx->comm, (int)world, u, (int)rank);
    if (r != ncclSuccess) {
        delete ctx;
        return fail("ncclCommInitRank(world %u, rank %u): %s", world, rank, g_rccl.error_string(r));
    }
    comm->rank = rank;
    comm->world = world;
    comm->ctx = ctx;
    comm->exchange = zkgpu_host::rccl_exchange;
    comm->abort = zkgpu_host::rccl_abort;
    return 0;
}

int zkgpu_comm_host_create(zkgpu_comm *comm, const char *name, uint32_t world, uint32_t rank, uint64_t capacity)
{
    return zkgpu_host::host_comm_create(comm, name, world, rank, capacity);
}

void zkgpu_comm_host_destroy(zkgpu_comm *comm) { zkgpu_host::host_comm_destroy(comm); }

void zkgpu_comm_rccl_destroy(zkgpu_comm *comm)
{
    if (!comm || !comm->ctx) return;
    auto *ctx = (zkgpu_host::RcclCtx *)comm->ctx;
    if (ctx->comm && !ctx->aborted && zkgpu_host::g_rccl.comm_destroy) zkgpu_host::g_rccl.comm_destroy(ctx->comm);
    if (ctx->done) (void)hipEventDestroy(ctx->done);
    delete ctx;
    comm->ctx = nullptr;
    comm->exchange = nullptr;
    comm->abort = nullptr;
}

}  // extern "C"
