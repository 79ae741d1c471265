// zkgpu_batch_prover -- the batch-proof STARK of Prover::genBatchProof
// (src/prover/prover.cpp:565-590) driven by the reference's own inputs:
//
//   config JSON (config.cpp:231-242 keys)
//     zkevmStarkInfo      <circuit>.starkinfo.json   (StarkInfo::load, stark_info.cpp:21-454)
//     zkevmConstPols      constant polynomials, N x nConstants u64 rows (starks.hpp:94-116)
//     zkevmConstantsTree  constant tree; its root must equal the tree built
//                         from zkevmConstPols (the prover's verkey)
//     zkevmCmPols         committed trace, N x nCm1 u64 rows (commit_pols.hpp)
//     zkevmVerkey         optional {"constRoot": [...]} checked like the tree
//     outputPath          directory for the outputs
//   --circuit <prefix> reads <prefix>StarkInfo / ConstPols / ConstantsTree /
//   Verkey / CmPols / Exec instead (config.cpp:243-259: c12a, recursive1,
//   recursive2, recursivef); the default prefix is zkevm.
//     <prefix>Exec        with --witness: the circuit's .exec file (execFile.hpp:48-64)
//     zkgpuPublics        the public inputs as a JSON array (the publics.json
//                         the reference writes, prover.cpp:657); genBatchProof
//                         computes them from the executor's Main columns
//                         (prover.cpp:480-560), which this driver does not run
//
//   outputs (json2file layout, utils.cpp:212-222)
//     <outputPath>/batch_proof.proof.json   FRIProof::proofs.proof2json() + "publics"
//     <outputPath>/batch_proof.zkin.json    proof2zkinStark() + "publics"
//
// The expression code comes from the starkinfo's step code (step2prev ...
// step52ns), run as GPU programs (ProverInfo, host/stark_info.cpp); for the
// zkEVM's parser bytecode, StepsGPU (host/zkgpu_steps.hpp) is the binding.
//
// Usage: zkgpu_batch_prover [--circuit PREFIX] [--witness FILE] [--stream-trace] [--check-trace] [--audit [--connections FILE]] [--shard RANK/WORLD --comm rccl:<id file>|host:</shm name> [--device D]]
//                           <config.json>
//        (--witness: the committed trace comes from a circom witness, a raw file of sizeWitness
//        little-endian u64 words, through <prefix>Exec on the GPU (zkgpu_stark_set_exec +
//        zkgpu_stark_set_cm1_witness: Circom*::getCommitedPols, prover.cpp:591-593, 629-630) in
//        place of the <prefix>CmPols file; .wtns parsing is not done here.  Single GPU; not with
//        --stream-trace; --audit and --check-trace work with it)
//        (--stream-trace: the trace file's rows stay in host memory and cross
//        PCIe under stage 1 of the proof, zkgpu_stark_prove_from_rows; single GPU)
//        (--check-trace: the constraint check in its STOP mode, zkgpu_stark_check_set:
//        a trace with a row that breaks the AIR ends the run before stage 3's
//        commit with the first such row in the message and the terms of the
//        constraint combination that fail there (zkgpu_stark_check_names_set),
//        a non-zero status and no proof files; single GPU)
//        (--audit: no proof.  The trace audit, zkgpu_stark_audit with naming on: every plookup
//        with values its table does not hold, every grand product that does not close and,
//        unless a plookup missed, every row that breaks an identity, each with its starkinfo
//        context; the report on stdout and in <outputPath>/trace_audit.json, no proof file;
//        status 0 for a clean trace, 3 for one with findings.  Not a verifier: the audit's
//        challenges do not depend on the trace (include/zkgpu_stark.h).  Single GPU)
//        (--connections FILE, with --audit: [{"ciCtx": i, "pols": [cm1 columns], "S": [constant
//        columns], "ks": [optional coset shifts]}] tells the columns of each connection check --
//        the starkinfo carries only expression ids -- so that an open connection product names
//        the cells that differ from the cell they are wired to (zkgpu_stark_conn_set): the lines
//        follow the product's in the report, with pols[i] beside the cm1 column, are repeated on
//        stderr, and trace_audit.json gains "connection" in the product's entry)
//        (--shard: one rank of ONE proof row-sharded over WORLD processes,
//        zkgpu_stark_create_sharded; every rank runs this command with the
//        same config, rank 0 writes the outputs.  rccl: rank 0 writes the
//        RCCL id to the file, the others wait for it; host: shared-memory
//        exchange for ranks sharing a GPU.  --device defaults to RANK for
//        rccl, 0 for host.)
//        zkgpu_batch_prover --info <starkinfo.json>                 (derived prover description; no GPU)
//        zkgpu_batch_prover --zkin <starkinfo.json> <flat proof> <publics.json> <outdir>
//                                                                   (proof JSON of a flat proof; no GPU)
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <fstream>
#include <map>
#include <memory>
#include <thread>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_stark.h"
#include "zkgpu_audit_format.hpp"
#include "zkgpu_fri_proof.hpp"
#include "zkgpu_json.hpp"
#include "zkgpu_stark_info.hpp"

using zkgpu::json::Value;

static std::string read_text(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f.good()) throw std::runtime_error("cannot open " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static std::vector<uint64_t> read_u64(const std::string &path, uint64_t expect)
{
    const std::string b = read_text(path);
    if (b.size() != expect * 8)
        throw std::runtime_error(path + ": " + std::to_string(b.size()) + " bytes, expected " + std::to_string(expect * 8));
    std::vector<uint64_t> v(expect);
    memcpy(v.data(), b.data(), b.size());
    return v;
}

static void write_json(const std::string &path, const Value &j)
{
    std::ofstream f(path, std::ios::binary);
    if (!f.good()) throw std::runtime_error("cannot create " + path);
    f << zkgpu::json::dump4(j) << "\n";
    if (!f.good()) throw std::runtime_error("write failed: " + path);
}

static std::vector<uint64_t> read_publics(const std::string &path, uint64_t n)
{
    const Value j = zkgpu::json::parse(read_text(path));
    if (j.size() != n) throw std::runtime_error(path + ": expected " + std::to_string(n) + " public inputs");
    std::vector<uint64_t> p(n);
    for (uint64_t i = 0; i < n; i++) p[i] = j[i].u64();
    return p;
}

static void write_outputs(const std::string &dir, const uint64_t *flat, uint64_t len, const zkgpu_stark_info &info,
                          const std::vector<uint64_t> &publics)
{
    mkdir(dir.c_str(), 0775);
    Value proof = zkgpu::proof2json(flat, len, info);
    Value zkin = zkgpu::proof2zkinStark(proof);
    Value pub = Value::array();
    for (uint64_t v : publics) pub.push(Value::str(std::to_string(v % 0xFFFFFFFF00000001ULL)));
    proof.set("publics", pub);  // prover.cpp:586-588
    zkin.set("publics", pub);
    write_json(dir + "/batch_proof.proof.json", proof);
    write_json(dir + "/batch_proof.zkin.json", zkin);
}

static uint64_t flat_len(const zkgpu_stark_info &in)
{
    // include/zkgpu_stark.h proof layout
    uint64_t L = 16 + 3ULL * in.n_ev;
    for (uint32_t si = 1; si < in.n_fri_steps; si++)
        L += 4 + (uint64_t)in.n_queries * (3ULL << (in.fri_steps[si - 1] - in.fri_steps[si])) +
             (uint64_t)in.n_queries * in.fri_steps[si] * 4;
    L += (uint64_t)in.n_queries * (in.n_cm1 + in.n_cm2 + in.n_cm3 + in.n_cm4 + in.n_const);
    L += 5ULL * in.n_queries * in.n_bits_ext * 4;
    L += 3ULL << in.fri_steps[in.n_fri_steps - 1];
    return L;
}

static void check_root(const std::string &what, const uint64_t got[4], const uint64_t want[4], const std::string &prefix)
{
    for (int i = 0; i < 4; i++)
        if (got[i] != want[i])
            throw std::runtime_error(what + ": constant root differs from the tree built from " + prefix + "ConstPols");
}

// a raw file of little-endian u64 words, whatever their number
static std::vector<uint64_t> read_u64_all(const std::string &path)
{
    const std::string b = read_text(path);
    if (b.size() % 8) throw std::runtime_error(path + ": " + std::to_string(b.size()) + " bytes, not whole u64 words");
    std::vector<uint64_t> v(b.size() / 8);
    if (!v.empty()) memcpy(v.data(), b.data(), b.size());
    return v;
}

struct Shard {
    uint32_t rank = 0, world = 1;
    std::string comm;  // "" (single GPU), "rccl:<file>", "host:<name>"
    int device = -1;
    bool stream_trace = false;  // --stream-trace: zkgpu_stark_prove_from_rows instead of set_cm1 + prove
    bool check_trace = false;   // --check-trace: zkgpu_stark_check_set(ZKGPU_CHECK_STOP)
    bool audit = false;         // --audit: zkgpu_stark_audit instead of a proof
    std::string circuit = "zkevm";  // --circuit: the prefix of the config keys
    std::string witness;            // --witness: a circom witness file through <prefix>Exec instead of <prefix>CmPols
    std::string connections;        // --connections: the wiring's columns of each ciCtx entry, for --audit
};

// --connections <file.json>: [{"ciCtx": i, "pols": [cm1 columns], "S": [constant columns], "ks": [optional]}].
// The starkinfo carries only expression ids under ciCtx, so the columns of the wiring are told here.
// Each entry declares its product (the driver's order puCtx, peCtx, ciCtx) a connection
// (zkgpu_stark_conn_set); returns product -> cm1 columns.  A malformed entry is refused by its index.
static std::map<uint32_t, std::vector<uint32_t>> declare_connections(void *h, const zkgpu::StarkInfo &si,
                                                                     const std::string &path)
{
    std::map<uint32_t, std::vector<uint32_t>> pols_of;
    const Value j = zkgpu::json::parse(read_text(path));
    if (j.kind != Value::Array) throw std::runtime_error("--connections: " + path + ": not a list of entries");
    for (size_t i = 0; i < j.size(); i++) {
        const std::string who = "--connections: entry " + std::to_string(i) + ": ";
        try {
            const Value &e = j[i];
            const uint64_t ci = e["ciCtx"].u64();
            if (ci >= si.ciCtx.size())
                throw std::runtime_error("ciCtx " + std::to_string(ci) + ": the starkinfo has " +
                                         std::to_string(si.ciCtx.size()) + " connection check(s)");
            const uint32_t z = (uint32_t)(si.puCtx.size() + si.peCtx.size() + ci);
            if (pols_of.count(z)) throw std::runtime_error("ciCtx " + std::to_string(ci) + " is declared twice");
            std::vector<uint32_t> pols, S;
            std::vector<uint64_t> ks;
            for (size_t k = 0; k < e["pols"].size(); k++) pols.push_back((uint32_t)e["pols"][k].u64());
            for (size_t k = 0; k < e["S"].size(); k++) S.push_back((uint32_t)e["S"][k].u64());
            if (e.contains("ks"))
                for (size_t k = 0; k < e["ks"].size(); k++) ks.push_back(e["ks"][k].u64());
            if (pols.empty() || pols.size() != S.size() || (e.contains("ks") && ks.size() != pols.size()))
                throw std::runtime_error("\"pols\", \"S\" and \"ks\" must be lists of one length, not empty (" +
                                         std::to_string(pols.size()) + ", " + std::to_string(S.size()) +
                                         (e.contains("ks") ? ", " + std::to_string(ks.size()) : "") + ")");
            const zkgpu_conn_desc d = {(uint32_t)pols.size(), pols.data(), S.data(), ks.empty() ? nullptr : ks.data()};
            if (zkgpu_stark_conn_set(h, z, &d)) throw std::runtime_error(zkgpu_stark_last_error());
            pols_of[z] = pols;
        } catch (const std::exception &x) {
            throw std::runtime_error(who + x.what());
        }
    }
    return pols_of;
}

// --audit: the report as text (stdout) and as <dir>/trace_audit.json, the keys of zkgpu_audit_report
// plus each finding's starkinfo context and, per listed failing row, the failing term ids.  The
// driver's products come in the order puCtx, peCtx, ciCtx: product k < nPu is plookup k's.
static int audit_trace(void *h, const zkgpu::StarkInfo &si, const zkgpu_stark_info &info, const std::string &dir,
                       const std::map<uint32_t, std::vector<uint32_t>> &conn_pols)
{
    zkgpu_audit_report r;
    if (zkgpu_stark_audit(h, ZKGPU_AUDIT_NAMES, &r)) throw std::runtime_error(std::string("audit: ") + zkgpu_stark_last_error());
    zkgpu_host::AuditContext c;
    c.n_bits = info.n_bits;
    c.n_pu = info.n_pu;
    c.n_zctx = info.n_zctx;
    for (uint32_t k = 0; k < info.n_pu; k++) c.pu_label.push_back(si.z_context(k));
    for (uint32_t z = 0; z < info.n_zctx; z++) {
        c.z_label.push_back(si.z_context(z));
        c.z_plookup.push_back(z < info.n_pu ? (int32_t)z : -1);
    }
    // a declared connection prints its cells as pols[i] beside the cm1 column
    for (const auto &kv : conn_pols) {
        if (c.conn_col_label.size() <= kv.first) c.conn_col_label.resize(kv.first + 1);
        for (size_t i = 0; i < kv.second.size(); i++)
            c.conn_col_label[kv.first].push_back("pols[" + std::to_string(i) + "] (cm1 column " +
                                                 std::to_string(kv.second[i]) + ")");
    }
    auto str = [](uint64_t v) { return Value::str(std::to_string(v % 0xFFFFFFFF00000001ULL)); };
    Value j = Value::object();
    j.set("clean", Value::num(r.clean));
    Value ch = Value::array();
    for (uint64_t v : r.challenges) ch.push(str(v));
    j.set("challenges", ch);
    j.set("n_pu_bad", Value::num(r.n_pu_bad));
    Value pus = Value::array();
    for (uint32_t k = 0; k < r.n_pu_bad && k < ZKGPU_AUDIT_MAX_PU; k++) {
        const zkgpu_audit_pu &e = r.pu[k];
        Value o = Value::object(), vals = Value::array();
        o.set("pu", Value::num(e.pu));
        o.set("context", Value::str(si.z_context(e.pu)));
        o.set("n_rows", Value::num(e.n_rows));
        o.set("n_vals", Value::num(e.n_vals));
        for (const zkgpu_lookup_miss &m : e.vals) {
            if (m.row == UINT64_MAX) break;
            Value p = Value::array();
            p.push(Value::num(m.row));
            p.push(Value::num(m.count));
            vals.push(p);
        }
        o.set("vals", vals);
        pus.push(o);
    }
    j.set("pu", pus);
    j.set("n_z_open", Value::num(r.n_z_open));
    Value zs = Value::array();
    for (uint32_t k = 0; k < r.n_z_open && k < ZKGPU_AUDIT_MAX_Z; k++) {
        const zkgpu_audit_z &e = r.z[k];
        Value o = Value::object();
        o.set("z", Value::num(e.z));
        o.set("context", Value::str(si.z_context(e.z)));
        o.set("compared", Value::num(e.compared));
        o.set("n_num", Value::num(e.n_num));
        o.set("n_den", Value::num(e.n_den));
        for (int side = 0; side < 2; side++) {
            Value l = Value::array();
            for (const zkgpu_z_diag_val &v : side ? e.den : e.num) {
                if (v.row == UINT64_MAX) break;
                Value t = Value::array();
                t.push(Value::num(v.row));
                t.push(Value::num(v.count_num));
                t.push(Value::num(v.count_den));
                l.push(t);
            }
            o.set(side ? "den" : "num", l);
        }
        // the cells a declared connection leaves unequal (zkgpu_stark_audit_conn), on stderr as well
        zkgpu_conn_report cr;
        if (zkgpu_stark_audit_conn(h, k, &cr)) throw std::runtime_error(std::string("audit: ") + zkgpu_stark_last_error());
        c.conn.push_back(cr);
        if (cr.ran) {
            Value q = Value::object(), br = Value::array(), fo = Value::array();
            q.set("n_broken", Value::num(cr.n_broken));
            q.set("n_foreign", Value::num(cr.n_foreign));
            q.set("n_untargeted", Value::num(cr.n_untargeted));
            for (const zkgpu_conn_break &b : cr.breaks) {
                if (b.row == UINT64_MAX) break;
                Value t = Value::array();
                t.push(Value::num(b.col));
                t.push(Value::num(b.row));
                t.push(Value::num(b.to_col));
                t.push(Value::num(b.to_row));
                t.push(str(b.value));
                t.push(str(b.to_value));
                br.push(t);
            }
            for (const zkgpu_conn_foreign &f : cr.foreign) {
                if (f.row == UINT64_MAX) break;
                Value t = Value::array();
                t.push(Value::num(f.col));
                t.push(Value::num(f.row));
                t.push(str(f.s_value));
                fo.push(t);
            }
            q.set("breaks", br);
            q.set("foreign", fo);
            o.set("connection", q);
            fprintf(stderr, "zkgpu_batch_prover: grand product %u is %s\n%s", e.z, si.z_context(e.z).c_str(),
                    zkgpu_host::audit_detail::conn_lines(
                        cr, e.z < c.conn_col_label.size() ? &c.conn_col_label[e.z] : nullptr).c_str());
        }
        zs.push(o);
    }
    j.set("z", zs);
    Value id = Value::object(), rows = Value::array(), val = Value::array(), al = Value::array(), named = Value::array();
    id.set("ran", Value::num(r.identities.ran));
    id.set("n_bad", Value::num(r.identities.n_bad));
    for (uint32_t s = 0; s < ZKGPU_CHECK_MAX_ROWS && r.identities.rows[s] != UINT64_MAX; s++) {
        rows.push(Value::num(r.identities.rows[s]));
        // the failing terms of the row (naming degrades to rows only when the split refuses the program)
        uint32_t n = 0;
        std::vector<uint32_t> ids(4096);
        std::vector<uint64_t> vals(3 * ids.size());
        if (!r.identities.ran || !r.identities.n_bad ||
            zkgpu_stark_check_named(h, s, ids.data(), vals.data(), (uint32_t)ids.size(), &n))
            continue;
        c.named = true;
        ids.resize(std::min<size_t>(n, ids.size()));
        Value t = Value::array();
        for (uint32_t x : ids) t.push(Value::num(x));
        named.push(t);
        c.term_ids.push_back(ids);
    }
    for (uint64_t v : r.identities.value) val.push(str(v));
    for (uint64_t v : r.identities.alpha) al.push(str(v));
    id.set("rows", rows);
    id.set("value", val);
    id.set("alpha", al);
    if (c.named) id.set("failing_terms", named);
    j.set("identities", id);
    printf("%s", zkgpu_host::audit_format(r, c).c_str());
    mkdir(dir.c_str(), 0775);
    write_json(dir + "/trace_audit.json", j);
    return r.clean ? 0 : 3;
}

// The RCCL id through a file: rank 0 writes it (atomic rename), the others
// poll.  Every file carries this run's tag -- ZKGPU_RUN_ID if set, else the
// launcher's pid (ranks started by one launcher share their parent) -- and a
// reader takes only a file with its own tag, so a file left by an earlier run
// at the same path is never mistaken for this run's id.  Rank 0 removes the
// file once the communicator exists (every rank has read it by then).
static std::string run_tag()
{
    const char *e = getenv("ZKGPU_RUN_ID");
    return e && *e ? std::string(e) : "ppid" + std::to_string((long)getppid());
}

static const char RCCL_ID_MAGIC[8] = {'Z', 'K', 'G', 'P', 'U', 'I', 'D', '1'};

static void rccl_id_file(const std::string &path, uint32_t rank, uint8_t id[128])
{
    const std::string tag = run_tag();
    if (rank == 0) {
        if (zkgpu_comm_rccl_unique_id(id)) throw std::runtime_error(std::string("rccl id: ") + zkgpu_stark_last_error());
        const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
        std::ofstream f(tmp, std::ios::binary);
        const uint32_t n = (uint32_t)tag.size();
        f.write(RCCL_ID_MAGIC, 8);
        f.write((const char *)&n, 4);
        f.write(tag.data(), n);
        f.write((const char *)id, 128);
        f.close();
        if (!f.good() || std::rename(tmp.c_str(), path.c_str())) throw std::runtime_error("cannot write " + path);
        return;
    }
    for (int t = 0; t < 6000; t++) {
        std::ifstream f(path, std::ios::binary);
        char magic[8];
        uint32_t n = 0;
        if (f.good() && f.read(magic, 8) && !memcmp(magic, RCCL_ID_MAGIC, 8) && f.read((char *)&n, 4) && n < 4096) {
            std::string got(n, '\0');
            if (f.read(&got[0], n) && got == tag && f.read((char *)id, 128) && f.gcount() == 128) return;
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(10));
    }
    throw std::runtime_error("no RCCL id for run " + tag + " in " + path + " after 60 s");
}

static int prove(const std::string &config_path, const Shard &sh)
{
    const Value cfg = zkgpu::json::parse(read_text(config_path));
    auto key = [&](const char *k) { return cfg[k].string(); };
    auto ckey = [&](const char *k) { return cfg[sh.circuit + k].string(); };  // the circuit's own files
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const zkgpu::StarkInfo si = zkgpu::StarkInfo::from_file(ckey("StarkInfo"));
    const zkgpu::ProverInfo pinfo(si);
    const zkgpu_stark_info &info = pinfo.info();
    const uint64_t N = 1ULL << info.n_bits;
    const std::vector<uint64_t> consts = read_u64(ckey("ConstPols"), N * info.n_const);
    const bool from_witness = !sh.witness.empty();
    std::vector<uint64_t> cm1, witness, exec_image;
    if (from_witness) {
        exec_image = read_u64_all(ckey("Exec"));
        witness = read_u64_all(sh.witness);
        if (witness.empty()) throw std::runtime_error(sh.witness + ": an empty witness");
    } else {
        cm1 = read_u64(ckey("CmPols"), N * info.n_cm1);
    }
    std::vector<uint64_t> publics(info.n_publics, 0);
    if (info.n_publics) publics = read_publics(key("zkgpuPublics"), info.n_publics);

    void *h = nullptr;
    zkgpu_comm comm{};
    struct CommGuard {
        zkgpu_comm *c;
        bool host;
        ~CommGuard()
        {
            if (host)
                zkgpu_comm_host_destroy(c);
            else
                zkgpu_comm_rccl_destroy(c);
        }
    };
    std::unique_ptr<CommGuard> comm_guard;
    if (sh.comm.empty()) {
        if (sh.device >= 0 && zkgpu_init(sh.device)) throw std::runtime_error(std::string("init: ") + zkgpu_last_error());
        if (zkgpu_stark_create(&h, &info)) throw std::runtime_error(std::string("create: ") + zkgpu_stark_last_error());
    } else {
        const bool host = sh.comm.rfind("host:", 0) == 0;
        const int dev = sh.device >= 0 ? sh.device : (host ? 0 : (int)sh.rank);
        if (zkgpu_init(dev)) throw std::runtime_error(std::string("init: ") + zkgpu_last_error());
        int rc;
        if (host) {
            rc = zkgpu_comm_host_create(&comm, sh.comm.c_str() + 5, sh.world, sh.rank, 1ULL << 30);
        } else if (sh.comm.rfind("rccl:", 0) == 0) {
            uint8_t id[128];
            rccl_id_file(sh.comm.substr(5), sh.rank, id);
            rc = zkgpu_comm_rccl_create(&comm, id, sh.world, sh.rank);
            if (!rc && sh.rank == 0) std::remove(sh.comm.substr(5).c_str());  // every rank has joined
        } else {
            throw std::runtime_error("--comm must be rccl:<file> or host:</name>");
        }
        if (rc) throw std::runtime_error(std::string("comm: ") + zkgpu_stark_last_error());
        comm_guard.reset(new CommGuard{&comm, host});
        if (zkgpu_stark_create_sharded(&h, &info, &comm))
            throw std::runtime_error(std::string("create: ") + zkgpu_stark_last_error());
    }
    struct Guard {
        void *h;
        ~Guard() { zkgpu_stark_destroy(h); }
    } guard{h};
    // (--stream-trace: the trace stays in host memory until the proof loads it under stage 1)
    if (zkgpu_stark_set_const(h, consts.data()) ||
        (from_witness && (zkgpu_stark_set_exec(h, exec_image.data(), exec_image.size(), witness.size()) ||
                          zkgpu_stark_set_cm1_witness(h, witness.data()))) ||
        (!from_witness && !sh.stream_trace && zkgpu_stark_set_cm1(h, cm1.data())) ||
        zkgpu_stark_set_publics(h, publics.data()))
        throw std::runtime_error(std::string("load: ") + zkgpu_stark_last_error());
    uint64_t verkey[4];
    zkgpu_stark_verkey(h, verkey);
    {
        // constant tree file: header, LDE, nodes; the root is its last 4 elements
        const std::string t = read_text(ckey("ConstantsTree"));
        if (t.size() < 32 || t.size() % 8) throw std::runtime_error(sh.circuit + "ConstantsTree: bad size");
        uint64_t root[4];
        memcpy(root, t.data() + t.size() - 32, 32);
        check_root(sh.circuit + "ConstantsTree", root, verkey, sh.circuit);
    }
    if (cfg.contains(sh.circuit + "Verkey")) {
        const Value vk = zkgpu::json::parse(read_text(ckey("Verkey")));
        uint64_t root[4];
        for (int i = 0; i < 4; i++) root[i] = vk["constRoot"][i].u64();
        check_root(sh.circuit + "Verkey", root, verkey, sh.circuit);
    }
    if (sh.check_trace && zkgpu_stark_check_set(h, ZKGPU_CHECK_STOP))
        throw std::runtime_error(std::string("--check-trace: ") + zkgpu_stark_last_error());
    // the failing identities with the failing rows; a quotient program the split refuses: rows only
    if (sh.check_trace && zkgpu_stark_check_names_set(h, 1))
        fprintf(stderr, "--check-trace: %s; the failing rows will be named, not the identities\n",
                zkgpu_stark_last_error());
    if (sh.audit) {
        std::map<uint32_t, std::vector<uint32_t>> conn_pols;
        if (!sh.connections.empty()) conn_pols = declare_connections(h, si, sh.connections);
        return audit_trace(h, si, info, key("outputPath"), conn_pols);
    }
    const auto t1 = clk::now();
    const uint64_t len = zkgpu_stark_proof_len(h);
    if (len != flat_len(info)) throw std::runtime_error("proof length mismatch");
    std::vector<uint64_t> flat(len);
    if (sh.stream_trace ? zkgpu_stark_prove_from_rows(h, cm1.data(), 1, flat.data()) : zkgpu_stark_prove(h, flat.data())) {
        // a grand product that does not close (no proof file is written): the diagnosis is in the
        // message; which context of the starkinfo the product is, from the order of the triples
        std::string msg = std::string("prove: ") + zkgpu_stark_last_error();
        zkgpu_z_diag zd;
        if (sh.comm.empty() && !zkgpu_stark_z_diag(h, &zd) && zd.n_open)
            msg += "; grand product " + std::to_string(zd.z) + " is " + si.z_context(zd.z);
        throw std::runtime_error(msg);
    }
    const auto t2 = clk::now();
    if (sh.rank == 0) write_outputs(key("outputPath"), flat.data(), len, info, publics);
    const auto t3 = clk::now();
    auto ms = [](clk::duration d) { return std::chrono::duration<double, std::milli>(d).count(); };
    fprintf(stderr, "zkgpu_batch_prover[%u/%u]: load %.1f ms, STARK_PROOF_BATCH_PROOF %.1f ms, json %.1f ms\n", sh.rank,
            sh.world, ms(t1 - t0), ms(t2 - t1), ms(t3 - t2));
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 3 && !strcmp(argv[1], "--info")) {
            const zkgpu::StarkInfo si = zkgpu::StarkInfo::from_file(argv[2]);
            printf("%s\n", zkgpu::json::dump4(zkgpu::ProverInfo(si).to_json()).c_str());
            return 0;
        }
        if (argc == 6 && !strcmp(argv[1], "--zkin")) {
            const zkgpu::StarkInfo si = zkgpu::StarkInfo::from_file(argv[2]);
            const zkgpu::ProverInfo pinfo(si);
            const uint64_t len = flat_len(pinfo.info());
            const std::vector<uint64_t> flat = read_u64(argv[3], len);
            write_outputs(argv[5], flat.data(), len, pinfo.info(), read_publics(argv[4], si.nPublics));
            return 0;
        }
        Shard sh;
        int a = 1;
        while (a + 1 < argc && argv[a][0] == '-' && argv[a][1] == '-') {
            const std::string opt = argv[a];
            if (opt == "--stream-trace") {
                sh.stream_trace = true;
                a += 1;
                continue;
            }
            if (opt == "--check-trace") {
                sh.check_trace = true;
                a += 1;
                continue;
            }
            if (opt == "--audit") {
                sh.audit = true;
                a += 1;
                continue;
            }
            if (opt == "--shard") {
                unsigned r = 0, w = 0;
                if (sscanf(argv[a + 1], "%u/%u", &r, &w) != 2 || !w || r >= w)
                    throw std::runtime_error("--shard takes RANK/WORLD");
                sh.rank = r;
                sh.world = w;
            } else if (opt == "--comm") {
                sh.comm = argv[a + 1];
            } else if (opt == "--device") {
                sh.device = atoi(argv[a + 1]);
            } else if (opt == "--circuit") {
                sh.circuit = argv[a + 1];
            } else if (opt == "--witness") {
                sh.witness = argv[a + 1];
            } else if (opt == "--connections") {
                sh.connections = argv[a + 1];
            } else {
                break;
            }
            a += 2;
        }
        if (sh.world > 1 && sh.comm.empty())
            throw std::runtime_error("--shard with WORLD > 1 needs --comm");
        if (sh.stream_trace && !sh.comm.empty())
            throw std::runtime_error("--stream-trace is for the single-GPU prover (no --comm)");
        if (!sh.witness.empty() && sh.stream_trace)
            throw std::runtime_error("--witness loads the trace on the GPU: not with --stream-trace (which streams the CmPols file)");
        if (!sh.witness.empty() && (sh.world > 1 || !sh.comm.empty()))
            throw std::runtime_error("--witness is for the single-GPU prover (not with --shard at WORLD > 1 or --comm)");
        if (sh.check_trace && sh.world > 1)
            throw std::runtime_error("--check-trace is for the single-GPU prover (not with --shard at WORLD > 1)");
        if (sh.audit && (sh.world > 1 || !sh.comm.empty()))
            throw std::runtime_error("--audit is for the single-GPU prover (not with --shard at WORLD > 1 or --comm)");
        if (sh.audit && (sh.stream_trace || sh.check_trace))
            throw std::runtime_error("--audit runs no proof: not with --stream-trace or --check-trace");
        if (!sh.connections.empty() && !sh.audit)
            throw std::runtime_error("--connections names the wiring for --audit: not without it");
        if (argc == a + 1 && argv[a][0] != '-') return prove(argv[a], sh);
        fprintf(stderr,
                "usage: %s [--circuit PREFIX] [--witness FILE] [--stream-trace] [--check-trace] [--audit [--connections FILE]] [--shard RANK/WORLD --comm rccl:<file>|host:</name> [--device D]] "
                "<config.json>\n"
                "       %s --info <starkinfo.json>\n"
                "       %s --zkin <starkinfo.json> <flat proof> <publics.json> <outdir>\n",
                argv[0], argv[0], argv[0]);
        return 2;
    } catch (const std::exception &e) {
        fprintf(stderr, "zkgpu_batch_prover: %s\n", e.what());
        return 1;
    }
}
