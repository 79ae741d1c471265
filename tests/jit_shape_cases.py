"""Two-instruction programs at the edge of what the expression-kernel source
generator (csrc/zxp_jit_source.cpp) prints: the two shapes it leaves to the
interpreter, and for each the neighbouring program it does print."""
from zkgpu.synthetic import Program, ADD, MUL, SEC_CM1_N, SEC_CM2_N, SEC_CM3_N  # noqa: F401 (sections: re-exported)


def cross_row_read_after_write():
    """cm2[0] = cm1[0] cm1[1]; cm3[0] = cm2[0]' + cm1[2]: the next row's cell of
    a column this row wrote (only the unshifted cell is in a register)"""
    p = Program(0)
    p.op(MUL, p.col(SEC_CM2_N, 0), p.col(SEC_CM1_N, 0), p.col(SEC_CM1_N, 1))
    p.op(ADD, p.col(SEC_CM3_N, 0), p.col(SEC_CM2_N, 0, 1), p.col(SEC_CM1_N, 2))
    return p


def cross_row_read_before_write():
    """the same read placed before the write: it sees the old value (not printed
    either: the generator decides by column, not by order)"""
    p = Program(0)
    p.op(ADD, p.col(SEC_CM3_N, 0), p.col(SEC_CM2_N, 0, 1), p.col(SEC_CM1_N, 2))
    p.op(MUL, p.col(SEC_CM2_N, 0), p.col(SEC_CM1_N, 0), p.col(SEC_CM1_N, 1))
    return p


def mixed_stored_triple():
    """cm3[3] = cm2[1] + cm1[2]; cm2[0..2] = cm1[0..2] chal0: a stored triple
    whose middle column the program reads and whose outer ones it does not"""
    p = Program(0)
    p.op(ADD, p.col(SEC_CM3_N, 3), p.col(SEC_CM2_N, 1), p.col(SEC_CM1_N, 2))
    p.op(MUL, p.col3(SEC_CM2_N, 0), p.col3(SEC_CM1_N, 0), p.chal(0))
    return p


def shifted_store_never_read():
    """cm2[0]' = cm1[0] cm1[1]; cm3[0] = cm1[1] + cm1[2]: a store to the next
    row of a column the program never reads"""
    p = Program(0)
    p.op(MUL, p.col(SEC_CM2_N, 0, 1), p.col(SEC_CM1_N, 0), p.col(SEC_CM1_N, 1))
    p.op(ADD, p.col(SEC_CM3_N, 0), p.col(SEC_CM1_N, 1), p.col(SEC_CM1_N, 2))
    return p


def shifted_store_read_back():
    """cm2[0]' = cm1[0] cm1[1]; cm3[0] = cm2[0]' + cm1[2]: the next row's cell
    read back in the row that wrote it (forwarded by the compiler)"""
    p = Program(0)
    p.op(MUL, p.col(SEC_CM2_N, 0, 1), p.col(SEC_CM1_N, 0), p.col(SEC_CM1_N, 1))
    p.op(ADD, p.col(SEC_CM3_N, 0), p.col(SEC_CM2_N, 0, 1), p.col(SEC_CM1_N, 2))
    return p


UNSUPPORTED = {"cross_row_read_after_write": cross_row_read_after_write, "mixed_stored_triple": mixed_stored_triple}
PRINTED = {"shifted_store_never_read": shifted_store_never_read, "shifted_store_read_back": shifted_store_read_back}
# section widths the four programs touch (cm1, cm2, cm3)
WIDTHS = {SEC_CM1_N: 3, SEC_CM2_N: 3, SEC_CM3_N: 4}
