"""ctypes mirrors of the assembly graph structs of include/oatk_syncasm.h (tests of the coverage estimates from read alignments)"""
import ctypes as C


class Arc(C.Structure):
    """oatk_asmg_arc_t (include/oatk_syncasm.h)"""
    _fields_ = [("v", C.c_uint64), ("w", C.c_uint64), ("ln", C.c_uint64), ("ls", C.c_uint64), ("cov", C.c_uint32, 30), ("del_", C.c_uint32, 1),
                ("comp", C.c_uint32, 1), ("link_id", C.c_uint64)]


class Vtx(C.Structure):
    """oatk_asmg_vtx_t"""
    _fields_ = [("n", C.c_uint64), ("a", C.c_void_p), ("seq", C.c_void_p), ("len", C.c_uint64), ("cov", C.c_uint32, 30), ("del_", C.c_uint32, 1),
                ("circ", C.c_uint32, 1)]


class Asmg(C.Structure):
    """oatk_asmg_t"""
    _fields_ = [("n_vtx", C.c_uint64), ("m_vtx", C.c_uint64), ("vtx", C.POINTER(Vtx)), ("n_arc", C.c_uint64), ("m_arc", C.c_uint64),
                ("arc", C.POINTER(Arc)), ("idx_p", C.c_void_p), ("idx_n", C.c_void_p)]


class Scg(C.Structure):
    """oatk_scg_t"""
    _fields_ = [("scm_db", C.c_void_p), ("utg_asmg", C.POINTER(Asmg)), ("scm_u", C.c_void_p), ("idx_u", C.c_void_p)]
