"""The trace audit (include/zkgpu_stark.h zkgpu_stark_audit) restated on the
CPU oracle, from what oracle/ and the other case modules already export: the
transcript, the stage programs and calculateZ of an OracleStark, oc.h1h2 where
Python has found no miss (lookup_cases), the multiset comparison
(multiset_cases), the n-domain constraint program (check_cases) and its split
into terms (split_cases).

audit(ostark, names) runs on the trace in ostark.S[0] and returns the dict of
GpuStark.audit() -- with names, also "named": per listed failing row the (ids,
values) of the live terms that are not zero there.  Faults: plant(trace, ...)
returns an altered copy of a clean SyntheticStark trace."""
import ctypes

import numpy as np

import check_cases as cc
import lookup_cases as lc
import multiset_cases as mc
import split_cases as sc

P = cc.P
MAX_PU, MAX_Z, MISS_MAX, Z_MAX = 8, 8, 16, 16


def challenges(ostark):
    """the audit's own: a transcript of the verkey and the publics, no root -> (8, 3) with ch0..ch3 and
    the combination challenge at index 4"""
    from oracle import oracle as oc
    t = oc.Transcript()
    t.put(ostark.verkey)
    t.put(ostark.publics)
    ch = np.zeros((8, 3), np.uint64)
    for k in range(5):
        ch[k] = t.get_field()
    return ch


def audit(ostark, names=False):
    from oracle import oracle as oc
    inst, N, S = ostark.inst, ostark.N, ostark.S
    zero3 = np.zeros(3, np.uint64)
    for s in (1, 2, 3):  # a column no stage writes reads 0
        S[s][:] = 0
    ch = challenges(ostark)
    rep = {"challenges": [int(x) for x in ch[:5].reshape(-1)]}
    # layer A
    ostark.run(inst.programs["step2"], ch, zero3)
    pus = []
    for k, (f_c, t_c, h1_c, h2_c, d) in enumerate(inst.pu):
        fcol = np.ascontiguousarray(S[3][:, f_c:f_c + d])
        tcol = np.ascontiguousarray(S[3][:, t_c:t_c + d])
        n_rows, n_vals, vals = lc.reference(fcol.T, tcol.T, MISS_MAX)
        if n_rows:
            S[1][:, h1_c:h1_c + d] = 0
            S[1][:, h2_c:h2_c + d] = 0
            pus.append({"pu": k, "n_rows": n_rows, "n_vals": n_vals, "vals": vals})
            continue
        h1, h2 = oc.h1h2(fcol.reshape(-1) if d == 1 else fcol, tcol.reshape(-1) if d == 1 else tcol)
        S[1][:, h1_c:h1_c + d] = h1.reshape(N, d)
        S[1][:, h2_c:h2_c + d] = h2.reshape(N, d)
    rep["n_pu_bad"], rep["pu"] = len(pus), pus[:MAX_PU]
    # layer B
    ostark.run(inst.programs["step3prev"], ch, zero3)
    zs = []
    u64p = ctypes.POINTER(ctypes.c_uint64)
    for z, (num_c, den_c, z_c) in enumerate(inst.z_ctx):
        zc = np.zeros((N, 3), np.uint64)
        num = np.ascontiguousarray(S[3][:, num_c:num_c + 3])
        den = np.ascontiguousarray(S[3][:, den_c:den_c + 3])
        ok = oc.lib().oc_calculate_z(zc.ctypes.data_as(u64p), 3, num.ctypes.data_as(u64p), 3,
                                     den.ctypes.data_as(u64p), 3, N)
        S[2][:, z_c:z_c + 3] = zc  # written whether or not the product closes
        if not ok:
            n_a, la, n_b, lb = mc.reference(num.T, den.T, Z_MAX)
            zs.append({"z": z, "compared": 1, "n_num": n_a, "n_den": n_b, "num": la, "den": lb})
    rep["n_z_open"], rep["z"] = len(zs), zs[:MAX_Z]
    # layer C
    ident = {"ran": 0, "n_bad": 0, "rows": [], "value": [0, 0, 0], "alpha": [int(x) for x in ch[4]]}
    if not pus:
        if inst.programs.get("step3") is not None and inst.programs["step3"].instr:
            ostark.run(inst.programs["step3"], ch, zero3)
        S[cc.SEC_Q_2NS] = np.zeros((N, 3), np.uint64)
        ostark.run(cc.NDomainProgram(inst.programs["step42ns"], inst.blowup_bits), ch, zero3)
        c = S[cc.SEC_Q_2NS] % np.uint64(P)
        bad = np.flatnonzero(c.any(axis=1))
        ident.update(ran=1, n_bad=int(bad.size), rows=[int(r) for r in bad[:cc.MAX_ROWS]],
                     value=[int(v) for v in c[bad[0]]] if bad.size else [0, 0, 0])
        if names and bad.size:
            tp = sc.TappedProgram(inst.programs["step42ns"], inst.blowup_bits)
            k = tp.terms.shape[0]
            S[cc.SEC_Q_2NS] = np.zeros((N, 3 * max(k, 1)), np.uint64)
            ostark.run(tp, ch, zero3)
            v = (S[cc.SEC_Q_2NS] % np.uint64(P)).reshape(N, max(k, 1), 3)[:, :k]
            rep["named"] = [sc.named(tp.terms, v, r) for r in ident["rows"]]
        elif names:
            rep["named"] = []
        del S[cc.SEC_Q_2NS]
    rep["identities"] = ident
    rep["clean"] = int(not pus and not zs and ident["ran"] == 1 and ident["n_bad"] == 0)
    return rep


def same_findings(got, want):
    """a GpuStark.audit() dict against the reference's: every key of the struct"""
    keys = ("clean", "challenges", "n_pu_bad", "pu", "n_z_open", "z", "identities")
    return {k: got[k] for k in keys} == {k: want[k] for k in keys}


# ---------------------------------------------------------------- planted faults
def absent_value(inst, ostark):
    """a base-field value no row of any lookup table holds"""
    have = set()
    for c in inst.c_t:
        have |= set(int(x) for x in ostark.S[4][:, c])
    v = 12345
    while v in have:
        v += 1
    return v


def plant(inst, trace, identity_rows=(), perm_cells=(), lookup_cells=()):
    """an altered copy of a clean trace:
    identity_rows  check_cases.corrupt's column (a2 of triple 0) + 1 at these rows
    perm_cells     (row, index into the permutation's A B C D) + 1
    lookup_cells   (plookup, row, value): every source column of the plookup set to the value there, so
                   that two rows given one value hold one tuple"""
    bad = trace.copy()
    for r in identity_rows:
        bad[r, 2] = (int(bad[r, 2]) + 1) % P
    for r, k in perm_cells:
        c = inst.perms[0]["cols"][k]
        bad[r, c] = (int(bad[r, c]) + 1) % P
    for pu, r, v in lookup_cells:
        for c in lookup_source_columns(inst, pu):
            bad[r, c] = v
    return bad


def lookup_source_columns(inst, pu):
    """plookup 0 looks (A, B) up in (T0, T1), plookup 1 looks C up in T2 (zkgpu/synthetic.py)"""
    return inst.cm1_lk[:2] if pu == 0 else inst.cm1_lk[2:3]
