"""ctypes binding of libcice4_amd.so (C-ABI in include/cice4_amd.h).

This is the Python stand-in for the Fortran ISO_C_BINDING shim
(cice4_amd/fortran/): same entry points, same argument order.  There is NO
CPU fallback: if the HIP library is missing or a device call fails, the call
raises.  Arrays are C-contiguous numpy arrays whose memory is the reference's
column-major layout: Fortran (nx,ny[,k][,nblocks]) <-> numpy ([nblocks,][k,] ny, nx).
"""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "libcice4_amd.so")
NCAT, NILYR, NSLYR, MAX_NTRCR = 5, 4, 1, 5

SIG_NAMES = ("stressp_1", "stressp_2", "stressp_3", "stressp_4", "stressm_1", "stressm_2",
             "stressm_3", "stressm_4", "stress12_1", "stress12_2", "stress12_3", "stress12_4")
EVP_GRID = ("dxt", "dyt", "dxhy", "dyhx", "cxp", "cyp", "cxm", "cym", "tarea", "uarea", "tarear",
            "uarear", "tinyarea", "fcor", "tmask", "umask")
EVP_GRID_OPT = ("HTN", "HTE")
EVP_IN = ("aice", "vice", "vsno", "aice0", "aicen", "vicen", "strairxT", "strairyT", "uocn", "vocn",
          "ss_tltx", "ss_tlty")
EVP_IO = ("uvel", "vvel") + SIG_NAMES + ("iceumask", "fm", "strtltx", "strtlty", "strocnx", "strocny",
                                          "strintx", "strinty")
EVP_OUT = ("strairx", "strairy", "strength", "divu", "shear", "rdg_conv", "rdg_shear", "prs_sig",
           "strocnxT", "strocnyT")
THERMO_STATE = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon")
THERMO_FORCING = ("flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot")
THERMO_CAT_IN = ("lhcoef", "shcoef")
THERMO_SW = ("fswsfc", "fswint", "fswthrun", "Sswabs", "Iswabs")
THERMO_OUT = ("fsurfn", "fcondtopn", "fsensn", "flatn", "fswabsn", "flwoutn", "evapn", "freshn",
              "fsaltn", "fhocnn", "meltt", "melts", "meltb", "congel", "snoice")
THERMO_ONSET = ("mlt_onset", "frz_onset")
THERMO_ARGS = THERMO_STATE + ("flw", "potT", "Qa", "rhoa", "fsnow", "fbot", "Tbot", "lhcoef",
                              "shcoef") + THERMO_SW + THERMO_OUT + THERMO_ONSET


class CiceError(RuntimeError):
    pass


class EvpGrid(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in EVP_GRID + EVP_GRID_OPT]


class EvpConfig(C.Structure):
    _fields_ = [("ndte", C.c_int), ("evp_damping", C.c_int), ("kstrength", C.c_int),
                ("krdg_partic", C.c_int), ("krdg_redist", C.c_int), ("mu_rdg", C.c_double)]


class EvpFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in EVP_IN + EVP_IO + EVP_OUT]


class ThermoConfig(C.Structure):
    _fields_ = [("heat_capacity", C.c_int), ("calc_Tsfc", C.c_int), ("conduct", C.c_int),
                ("ustar_min", C.c_double), ("tr_iage", C.c_int), ("nt_Tsfc", C.c_int),
                ("nt_iage", C.c_int)]


MERGE_ORDER = ("strairxT", "strairyT", "fsurf", "fcondtop", "fsens", "flat", "fswabs", "flwout", "evap", "Tref",
               "Qref", "fresh", "fsalt", "fhocn", "fswthru", "meltt", "meltb", "melts", "congel", "snoice")


class MergeFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("aicen_init", "strairxn", "strairyn", "Trefn", "Qrefn")] + \
               [("acc", C.c_void_p * 20)]


class TransportConfig(C.Structure):
    _fields_ = [("ntrcr", C.c_int), ("trcr_depend", C.c_int * 5)]


class TransportGrid(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("HTN", "HTE", "dxt", "dyt", "dxu", "dyu", "tarear", "hm")]


class TransportFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("aice0", "aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "uvel", "vvel")]


class FrzmltFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("aice", "frzmlt", "sst", "Tf", "strocnxT", "strocnyT", "Tbot", "fbot", "rside")]


class AtmoFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("uatm", "vatm", "wind", "zlvl", "strax", "stray")] + \
               [("calc_strair", C.c_int)] + \
               [(n, C.c_void_p) for n in ("strairxn", "strairyn", "Trefn", "Qrefn", "lhcoef", "shcoef")]


class ItdConfig(C.Structure):
    _fields_ = [("ntrcr", C.c_int), ("trcr_depend", C.c_int * 5), ("nt_Tsfc", C.c_int), ("nt_iage", C.c_int),
                ("nt_alvl", C.c_int), ("nt_vlvl", C.c_int), ("tr_iage", C.c_int), ("tr_lvl", C.c_int),
                ("update_ocn_f", C.c_int), ("hin_max", C.c_double * 6), ("hi_min", C.c_double)]


THERM2_PTRS = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "aicen_init", "vicen_init", "frain", "frzmlt", "Tf",
               "rside", "tmask", "aice", "aice0", "fresh", "fsalt", "fhocn", "frazil", "meltl", "frz_onset")


class Therm2Fields(C.Structure):
    _fields_ = [("ncat", C.c_int), ("kitd", C.c_int), ("state_resident", C.c_int)] + [(n, C.c_void_p) for n in THERM2_PTRS]


CLEANUP_PTRS = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "tmask", "aice", "aice0", "vice", "vsno", "eice", "esno",
                "trcr", "fresh", "fsalt", "fhocn", "daidtt", "dvidtt")
CLEANUP_TIMES = ("head",) + tuple(f"pass{p}" for p in range(1, 9)) + ("zap", "bound_state", "aggregate")


class Therm2CleanupFields(C.Structure):
    _fields_ = [("ncat", C.c_int), ("state_resident", C.c_int), ("bound", C.c_int)] + [(n, C.c_void_p) for n in CLEANUP_PTRS]


RIDGE_PTRS = ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "tmask", "rdg_conv", "rdg_shear", "aice0", "dardg1dt",
              "dardg2dt", "dvirdgdt", "opening", "aice", "vice", "vsno", "eice", "esno", "trcr", "fresh", "fsalt", "fhocn",
              "daidtd", "dvidtd")
RIDGE_NITERMAX = 20
RIDGE_TIMES = tuple(f"{k}{i}" for i in range(1, RIDGE_NITERMAX + 1) for k in ("rates", "shift")) + ("finish",)


class RidgeFields(C.Structure):
    _fields_ = [("ncat", C.c_int), ("bound", C.c_int)] + [(n, C.c_void_p) for n in RIDGE_PTRS]


class ShortwaveConfig(C.Structure):
    _fields_ = [("shortwave", C.c_int), ("albedo_type", C.c_int)] + [
        (n, C.c_double) for n in ("albicev", "albicei", "albsnowv", "albsnowi", "ahmax", "albocn", "dT_mlt", "dalb_mlt",
                                  "snowpatch", "awtvdr", "awtidr", "awtvdf", "awtidf")]


RADIATION_STATE = ("aicen", "trcrn", "vicen", "vsnon")
RADIATION_IN = ("swvdr", "swvdf", "swidr", "swidf", "ocn_albedo")
RADIATION_OUT = ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "fswsfcn", "fswintn", "fswthrun", "Sswabsn",
                 "Iswabsn")
RADIATION_SW = ("fswsfcn", "fswintn", "fswthrun", "Sswabsn", "Iswabsn")
PREP_RADIATION_PTRS = ("swvdr", "swvdf", "swidr", "swidf", "alvdr_gbm", "alvdf_gbm", "alidr_gbm", "alidf_gbm", "aice",
                       "scale_factor", "fswfac") + RADIATION_SW + ("aicen",)


class RadiationFields(C.Structure):
    _fields_ = [("ncat", C.c_int), ("state_resident", C.c_int)] + [
        (n, C.c_void_p) for n in RADIATION_STATE + RADIATION_IN + RADIATION_OUT + ("coszen",)]


class DeddConfig(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("R_ice", "R_pnd", "R_snw", "awtvdr", "awtidr", "awtvdf", "awtidf")] + [
        ("tr_pond", C.c_int)]


RADIATION_DEDD_IN = ("swvdr", "swvdf", "swidr", "swidf", "coszen", "apondn", "hpondn")
RADIATION_DEDD_OUT = ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "albpndn", "fswsfcn", "fswintn", "fswthrun",
                      "Sswabsn", "Iswabsn")


class RadiationDeddFields(C.Structure):
    _fields_ = [("ncat", C.c_int), ("state_resident", C.c_int)] + [
        (n, C.c_void_p) for n in RADIATION_STATE + RADIATION_DEDD_IN + RADIATION_DEDD_OUT]


class PrepRadiationFields(C.Structure):
    _fields_ = [("ncat", C.c_int), ("sw_resident", C.c_int)] + [(n, C.c_void_p) for n in PREP_RADIATION_PTRS]


class CouplingConfig(C.Structure):
    _fields_ = [("scale_fluxes", C.c_int), ("oceanmixed_ice", C.c_int), ("atmbndy", C.c_int), ("albocn", C.c_double)]


# cice_coupling_fields in the order of the struct: tmask (int32), then doubles
COUPLING_CAT_IN = ("alvdrn", "alidrn", "alvdfn", "alidfn", "albicen", "albsnon", "albpndn", "aicen")
COUPLING_IN = ("coszen", "aice", "Tf", "Tair", "Qa", "swvdr", "swvdf", "swidr", "swidf")
COUPLING_FLUXES = ("strairxT", "strairyT", "fsens", "flat", "fswabs", "flwout", "evap", "Tref", "Qref", "fresh", "fsalt",
                   "fhocn", "fswthru")
COUPLING_OUT = ("alvdr", "alidr", "alvdf", "alidf", "albice", "albsno", "albpnd", "alvdf_gbm", "alidf_gbm", "alvdr_gbm",
                "alidr_gbm", "fresh_gbm", "fsalt_gbm", "fhocn_gbm", "fswthru_gbm", "scale_factor")
COUPLING_MIX_IN = ("potT", "uatm", "vatm", "wind", "zlvl", "rhoa", "flw", "hmix")
COUPLING_MIX_IO = ("sst", "qdp")
COUPLING_MIX_OUT = ("frzmlt", "flwout_ocn", "fsens_ocn", "flat_ocn", "evap_ocn", "strairx_ocn", "strairy_ocn", "Tref_ocn",
                    "Qref_ocn", "alvdr_ocn", "alidr_ocn", "alvdf_ocn", "alidf_ocn")
COUPLING_MIX_OPT = ("delt", "delq", "shcoef", "lhcoef")
COUPLING_PTRS = (COUPLING_CAT_IN + COUPLING_IN + COUPLING_FLUXES + COUPLING_OUT + ("albcnt",) + COUPLING_MIX_IN +
                 COUPLING_MIX_IO + COUPLING_MIX_OUT + COUPLING_MIX_OPT)


class CouplingFields(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("ncat", "state_resident", "alb_resident", "bound", "nstreams")] + [
        ("tmask", C.c_void_p)] + [(n, C.c_void_p) for n in COUPLING_PTRS]


# cice_pond_fields in the order of the struct
POND_PTRS = ("frain", "trcrn", "apondn", "hpondn", "aicen", "vicen", "vsnon", "melttn", "meltsn")


class PondFields(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("ncat", "state_resident", "ponds", "age")] + [(n, C.c_void_p) for n in POND_PTRS]


class ThermoFields(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in THERMO_STATE + THERMO_FORCING + THERMO_CAT_IN + THERMO_SW
                + THERMO_OUT + THERMO_ONSET]


_libs = {}


def load(flavour="standalone"):
    """Load the HIP library; raises if it has not been built (python -c 'import
    __graft_entry__ as g; g.build()' or make -C cice4_amd/csrc).  flavour "auscom": libcice4_amd_auscom.so, the
    build that replaces a reference compiled -DAusCOM -Dcoupled (include/cice4_amd.h: cice_build_flavour)."""
    if flavour not in _libs:
        if flavour not in ("standalone", "auscom"):
            raise CiceError(f"unknown flavour {flavour!r}")
        path = LIBPATH if flavour == "standalone" else LIBPATH.replace(".so", "_auscom.so")
        if not os.path.exists(path):
            raise CiceError(f"{path} not found: build the HIP extension first (make -C cice4_amd/csrc)")
        lib = C.CDLL(path)
        lib.cice_last_error.restype = C.c_char_p
        lib.cice_last_error.argtypes = [C.c_void_p]
        lib.cice_build_flavour.restype = C.c_char_p
        if lib.cice_build_flavour().decode() != flavour:
            raise CiceError(f"{path} reports flavour {lib.cice_build_flavour().decode()!r}")
        _libs[flavour] = lib
    return _libs[flavour]


def join_map(nxg, nyg, bsx, bsy, ew=1, ns=0, flavour="standalone", fold=False):
    """cice_debug_join_map (no device): the cell map of the image that a one-task domain in blocks of bsx x bsy is joined
    into for the K-subcycle sweeps (option "skew_join"), as an int32 array (nblocks, bsy + 2, bsx + 2) of 0-based cells of the
    row-major (nyg + 2) x (nxg + 2) image, -1 for padding; None if the layout does not qualify.  fold=True: the geometry of
    option "skew_join_fold", which admits a tripole north boundary (cice_debug_join_map_fold)."""
    L = load(flavour)
    fn = L.cice_debug_join_map_fold if fold else L.cice_debug_join_map
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_longlong]
    n = fn(nxg, nyg, bsx, bsy, ew, ns, None, 0)
    if n < 0:
        raise CiceError(f"cice_debug_join_map: bad arguments ({n})")
    if n == 0:
        return None
    m = np.full(n, -2, np.int32)
    assert fn(nxg, nyg, bsx, bsy, ew, ns, _i4(m), n) == n
    return m.reshape(-1, bsy + 2, bsx + 2)


def _p(a, dtype=None):
    if a is None:
        return None
    if dtype is not None and a.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {a.dtype}")
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return a.ctypes.data_as(C.c_void_p)


def _f8(a):
    return _p(a, np.float64)


def _i4(a):
    return _p(a, np.int32)


class Context:
    """One rank = one GPU (cice_ctx)."""

    def __init__(self, device=-1, flavour="standalone"):
        self.lib = load(flavour)
        self.flavour = flavour
        self.h = C.c_void_p()
        rc = self.lib.cice_create(C.byref(self.h), C.c_int(device))
        if rc:
            raise CiceError("cice_create failed")
        self.nx = self.ny = self.nblocks = 0
        self._keep = []

    def close(self):
        if self.h:
            self.lib.cice_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            msg = self.lib.cice_last_error(self.h)
            raise CiceError(f"cice4_amd error {rc}: {msg.decode() if msg else ''}")

    def sync(self):
        self._ck(self.lib.cice_device_sync(self.h))

    def set_auscom(self, cosw=1.0, sinw=0.0, dragio=0.00536, use_ocnslope=False):
        """flavour "auscom" only: the namelist variables of the coupled build's dynamics (cice_set_auscom)"""
        self._ck(self.lib.cice_set_auscom(self.h, C.c_double(cosw), C.c_double(sinw), C.c_double(dragio),
                                          C.c_int(int(use_ocnslope))))

    def set_chio(self, chio=0.006):
        """flavour "auscom" only: basal heat-transfer coefficient of frzmlt_bottom_lateral (cice_thermo_set_chio)"""
        self._ck(self.lib.cice_thermo_set_chio(self.h, C.c_double(chio)))

    def diag_stream_copy(self, n_doubles):
        ms = C.c_float(0.0)
        self._ck(self.lib.cice_diag_stream_copy(self.h, C.c_longlong(n_doubles), C.byref(ms)))
        return ms.value

    # ---- domain -------------------------------------------------------
    def domain_create(self, nxg, nyg, bsx, bsy, ew=1, ns=0, rank=0, npx=1, npy=1):
        self._ck(self.lib.cice_domain_create(self.h, nxg, nyg, bsx, bsy, ew, ns, rank, npx, npy))
        info = (C.c_int * 9)()
        self._ck(self.lib.cice_domain_info(self.h, info))
        self.nx, self.ny, self.nblocks = info[0], info[1], info[2]
        self.dinfo = dict(nx=info[0], ny=info[1], nblocks=info[2], nblocks_tot=info[3], ncopy=info[4],
                          nsend=info[5], nrecv=info[6], nsend_elems=info[7], nrecv_elems=info[8],
                          nxg=nxg, nyg=nyg)
        return self.domain()

    def domain_create_map(self, nxg, nyg, bsx, bsy, owner, ew=1, ns=0, rank=0, nranks=1, local_id=None):
        """Any block->task map; owner[g] = rank or -1 (eliminated land block)."""
        owner = np.ascontiguousarray(owner, np.int32)
        lid = None if local_id is None else np.ascontiguousarray(local_id, np.int32)
        self._ck(self.lib.cice_domain_create_map(self.h, nxg, nyg, bsx, bsy, ew, ns, rank, nranks, _i4(owner),
                                                 None if lid is None else _i4(lid)))
        info = (C.c_int * 9)()
        self._ck(self.lib.cice_domain_info(self.h, info))
        self.nx, self.ny, self.nblocks = info[0], info[1], info[2]
        self.dinfo = dict(nx=info[0], ny=info[1], nblocks=info[2], nblocks_tot=info[3], ncopy=info[4],
                          nsend=info[5], nrecv=info[6], nsend_elems=info[7], nrecv_elems=info[8],
                          nxg=nxg, nyg=nyg)
        return self.domain()

    def domain_list(self, name, loc=1):
        n = C.c_int(0)
        self._ck(self.lib.cice_domain_list(self.h, name.encode(), loc, C.byref(n), None))
        out = np.zeros(n.value, np.int32)
        if n.value:
            self._ck(self.lib.cice_domain_list(self.h, name.encode(), loc, C.byref(n), _i4(out)))
        return out

    def domain_create_slabs(self, nxg, nyg, nblocks_y, ew=1, ns=0, rank=0, nranks=1, overlap=0):
        """j-slabs of full width, optionally extended by `overlap` rows (wide halo)."""
        self._ck(self.lib.cice_domain_create_slabs(self.h, nxg, nyg, nblocks_y, ew, ns, rank, nranks, overlap))
        info = (C.c_int * 9)()
        self._ck(self.lib.cice_domain_info(self.h, info))
        self.nx, self.ny, self.nblocks = info[0], info[1], info[2]
        self.dinfo = dict(nx=info[0], ny=info[1], nblocks=info[2], nblocks_tot=info[3], ncopy=info[4],
                          nsend=info[5], nrecv=info[6], nsend_elems=info[7], nrecv_elems=info[8],
                          nxg=nxg, nyg=nyg, overlap=overlap)
        return self.domain()

    def domain(self):
        """dict describing the local blocks + on-rank halo list (host logic, no GPU needed)."""
        d = dict(self.dinfo)
        cols = {k: [] for k in ("ilo", "ihi", "jlo", "jhi", "i0", "j0", "gid", "owner", "own_jlo", "own_jhi")}
        for b in range(self.nblocks):
            info = (C.c_int * 10)()
            self._ck(self.lib.cice_domain_block(self.h, b, info))
            for k, v in zip(cols, info):
                cols[k].append(v)
        d.update({k: np.array(v, np.int32) for k, v in cols.items()})
        src = np.zeros(d["ncopy"], np.int32); dst = np.zeros(d["ncopy"], np.int32)
        if d["ncopy"]:
            self._ck(self.lib.cice_domain_halo_local(self.h, _i4(src), _i4(dst)))
        d["hsrc"], d["hdst"] = src, dst
        nr = C.c_int(0)
        self._ck(self.lib.cice_domain_halo_refresh(self.h, C.byref(nr), None, None))
        rs = np.zeros(nr.value, np.int32); rd = np.zeros(nr.value, np.int32)
        if nr.value:
            self._ck(self.lib.cice_domain_halo_refresh(self.h, C.byref(nr), _i4(rs), _i4(rd)))
        d["rsrc"], d["rdst"] = rs, rd
        d["hfill"] = self.domain_list("hfill")
        return d

    def apply_halo_lists(self, a, loc=1, kind=1, fill=0):
        """The halo update the device performs, in numpy on a host array (nlev?, nblocks, ny, nx) -- for CPU tests of
        the lists: on-rank copies, fill of ghost cells facing eliminated blocks, tripole fold (single-rank domains)."""
        d = self.domain()
        n = self.nblocks * self.ny * self.nx
        v = a.reshape(-1, n)
        v[:, d["hdst"]] = v[:, d["hsrc"]]
        if len(d["hfill"]):
            v[:, d["hfill"]] = fill
        lsrc, bidx = self.domain_list("fold_lsrc"), self.domain_list("fold_bidx")
        if len(lsrc):
            sgn = 1 if kind == 1 else -1
            rows = int(bidx.max()) // self.dinfo["nxg"] + 1     # 2: fold through U points, 3: through T points
            buf = np.full((v.shape[0], rows * self.dinfo["nxg"]), fill, a.dtype)
            buf[:, bidx] = v[:, lsrc]
            lo, hi = self.domain_list("fold_lo", loc), self.domain_list("fold_hi", loc)
            if len(lo):
                if a.dtype == np.int32:   # nint(0.5_dbl_kind*(x1 + isign*x2)), halves away from zero
                    t = 0.5 * (buf[:, lo] + sgn * buf[:, hi]).astype(np.float64)
                    x = (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int32)
                else:
                    x = (a.dtype.type(0.5) * (buf[:, lo] + a.dtype.type(sgn) * buf[:, hi])).astype(a.dtype)
                buf[:, lo] = x
                buf[:, hi] = a.dtype.type(sgn) * x
            dst, src = self.domain_list("fold_dst", loc), self.domain_list("fold_src", loc)
            v[:, dst] = a.dtype.type(sgn) * buf[:, src]
        return a

    def halo_msgs(self, direction):
        """direction 0 / 1: ghost-cell messages sent / received; 2 / 3: tripole top rows sent / received (receive
        addresses are indices into the global fold buffer).  The list ends at the first CICE_EINVAL for a message
        index; a context without a domain or a bad direction is an error, not an empty list, and for directions
        0 / 1 the count is checked against cice_domain_info."""
        if direction not in (0, 1, 2, 3):
            raise CiceError(f"halo_msgs: direction {direction} not in 0..3")
        if not getattr(self, "dinfo", None):
            raise CiceError("halo_msgs: no domain (call domain_create* first)")
        out = []
        m = -1
        while True:
            m += 1
            peer = C.c_int(); cnt = C.c_int()
            rc = self.lib.cice_domain_halo_msg(self.h, direction, m, C.byref(peer), C.byref(cnt), None)
            if rc == -1:        # CICE_EINVAL: past the last message (context and direction were checked above)
                break
            self._ck(rc)
            addr = np.zeros(cnt.value, np.int32)
            self._ck(self.lib.cice_domain_halo_msg(self.h, direction, m, None, None, _i4(addr)))
            out.append((peer.value, addr))
        if direction in (0, 1):
            want = self.dinfo["nsend" if direction == 0 else "nrecv"]
            if len(out) != want:
                raise CiceError(f"halo_msgs({direction}): {len(out)} messages listed, cice_domain_info says {want}")
        return out

    # ---- communication --------------------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        rc = self.lib.cice_comm_unique_id(buf)
        if rc:
            raise CiceError(f"cice_comm_unique_id failed ({rc})")
        return buf.raw

    def comm_init(self, uid, rank, nranks):
        self._ck(self.lib.cice_comm_init(self.h, C.c_char_p(uid), rank, nranks))

    def check_sizes(self, ncat, nilyr, nslyr, max_ntrcr):
        """CiceError unless the host model's ice_domain_size parameters are the library's compile-time sizes"""
        self._ck(self.lib.cice_check_sizes(self.h, ncat, nilyr, nslyr, max_ntrcr))

    def comm_init_local(self, link_id, rank, nranks):
        """in-process link instead of an RCCL communicator: the ranks are contexts of this process (tests)"""
        self._ck(self.lib.cice_comm_init_local(self.h, link_id, rank, nranks))

    def comm_init_shm(self, name, rank, nranks, box_bytes=64 << 20):
        """the same between processes of one host (a file under /dev/shm)"""
        self._ck(self.lib.cice_comm_init_shm(self.h, name.encode(), rank, nranks, C.c_longlong(box_bytes)))

    def comm_init_mirror(self, rank, nranks):
        """timing aid: this context is rank `rank` of `nranks`, alone on its device; its messages come back to it"""
        self._ck(self.lib.cice_comm_init_mirror(self.h, rank, nranks))

    def comm_count(self):
        """ranks of this context's communicator as RCCL counts them (0 before comm_init)"""
        n = C.c_int(0)
        self._ck(self.lib.cice_comm_count(self.h, C.byref(n)))
        return n.value

    # ---- EVP -----------------------------------------------------------------
    def evp_init(self, grid, ndte=120, evp_damping=False, kstrength=1, krdg_partic=1, krdg_redist=1,
                 mu_rdg=4.0):
        g = EvpGrid()
        for n in EVP_GRID:
            a = grid[n]
            setattr(g, n, (_i4(a) if n in ("tmask", "umask") else _f8(a)))
        for n in EVP_GRID_OPT:
            setattr(g, n, _f8(grid[n]) if n in grid else None)
        cfg = EvpConfig(ndte, int(evp_damping), kstrength, krdg_partic, krdg_redist, mu_rdg)
        self._ck(self.lib.cice_evp_init(self.h, C.byref(cfg), C.byref(g)))

    @staticmethod
    def _evp_fields(s, need_out=True):
        f = EvpFields()
        for n in EVP_IN + EVP_IO:
            if s.get(n) is None:          # left to the device (evp_adopt_thermo_state)
                setattr(f, n, None)
                continue
            setattr(f, n, (_i4(s[n]) if n == "iceumask" else _f8(s[n])))
        for n in EVP_OUT:
            setattr(f, n, _f8(s[n]) if (n in s) else None)
        return f

    def evp(self, dt, s):
        """Drop-in evp(dt): s holds the module arrays (modified in place)."""
        f = self._evp_fields(s)
        self._ck(self.lib.cice_evp(self.h, C.c_double(dt), C.byref(f)))

    def evp_adopt_thermo_state(self):
        """aicen, vicen (+ the aggregates) of the dynamics from the batched thermo state on the device; the next
        evp / evp_upload may leave aice, vice, vsno, aice0, aicen, vicen out (None)"""
        self._ck(self.lib.cice_evp_adopt_thermo_state(self.h))

    def evp_pin_fields(self, s):
        """Page-lock the arrays of s (they must stay alive and keep their addresses)."""
        f = self._evp_fields(s)
        self._ck(self.lib.cice_evp_pin_fields(self.h, C.byref(f)))

    def evp_upload(self, s):
        f = self._evp_fields(s)
        self._ck(self.lib.cice_evp_upload(self.h, C.byref(f)))

    def evp_download(self, s):
        f = self._evp_fields(s)
        self._ck(self.lib.cice_evp_download(self.h, C.byref(f)))

    def evp_download_stresses(self, s):
        f = self._evp_fields(s)
        self._ck(self.lib.cice_evp_download_stresses(self.h, C.byref(f)))

    def evp_step(self, dt):
        self._ck(self.lib.cice_evp_step(self.h, C.c_double(dt)))

    def evp_prepare(self, dt):
        self._ck(self.lib.cice_evp_prepare(self.h, C.c_double(dt)))

    def evp_subcycles(self, ksub0, nsub, timed=False):
        ms = C.c_float(0.0)
        self._ck(self.lib.cice_evp_subcycles(self.h, ksub0, nsub, C.byref(ms) if timed else None))
        return ms.value

    def evp_finish(self):
        self._ck(self.lib.cice_evp_finish(self.h))

    def evp_set_option(self, key, value):
        self._ck(self.lib.cice_evp_set_option(self.h, key.encode(), int(value)))

    def evp_get_info(self, key):
        v = C.c_int(0)
        self._ck(self.lib.cice_evp_get_info(self.h, key.encode(), C.byref(v)))
        return v.value

    def evp_peer_export(self):
        """(xu0, xu1, rprog, plane): device pointers of this rank's exchange copies / progress words and its plane size"""
        bufs = (C.c_void_p * 3)(); plane = C.c_longlong(0)
        self._ck(self.lib.cice_evp_peer_export(self.h, bufs, C.byref(plane)))
        return bufs[0], bufs[1], bufs[2], plane.value

    def evp_peer_connect(self, side, peer):
        """side 0: `peer` (an evp_peer_export tuple) is the rank to the south, 1: to the north"""
        self._ck(self.lib.cice_evp_peer_connect(self.h, side, C.c_void_p(peer[0]), C.c_void_p(peer[1]), C.c_void_p(peer[2]),
                                                C.c_longlong(peer[3])))

    def evp_peer_export_ipc(self):
        """(3 x 64-byte IPC handles, plane): the same buffers for a neighbour in another process"""
        h = C.create_string_buffer(192); plane = C.c_longlong(0)
        self._ck(self.lib.cice_evp_peer_export_ipc(self.h, h, C.byref(plane)))
        return h.raw, plane.value

    def evp_peer_connect_ipc(self, side, peer):
        self._ck(self.lib.cice_evp_peer_connect_ipc(self.h, side, C.c_char_p(peer[0]), C.c_longlong(peer[1])))

    def evp_peer_ranks(self):
        """the ranks this rank's block exchanges ghost cells with (ascending; any cartesian layout, one block per rank)"""
        n = C.c_int(0); r = (C.c_int32 * 8)()
        self._ck(self.lib.cice_evp_peer_ranks(self.h, C.byref(n), r))
        return [int(r[k]) for k in range(n.value)]

    def evp_peer_connect_rank(self, rank, peer):
        """`peer` (an evp_peer_export tuple) are the buffers of neighbouring rank `rank`"""
        self._ck(self.lib.cice_evp_peer_connect_rank(self.h, rank, C.c_void_p(peer[0]), C.c_void_p(peer[1]), C.c_void_p(peer[2]),
                                                     C.c_longlong(peer[3])))

    def evp_peer_connect_rank_ipc(self, rank, peer):
        self._ck(self.lib.cice_evp_peer_connect_rank_ipc(self.h, rank, C.c_char_p(peer[0]), C.c_longlong(peer[1])))

    def evp_debug(self, what):
        n = C.c_longlong(0)
        self._ck(self.lib.cice_evp_debug(self.h, what.encode(), None, C.byref(n)))
        out = np.zeros(n.value, np.int64)
        if n.value:
            self._ck(self.lib.cice_evp_debug(self.h, what.encode(), out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def evp_active_cells(self):
        nt = C.c_longlong(); nu = C.c_longlong()
        self._ck(self.lib.cice_evp_active_cells(self.h, C.byref(nt), C.byref(nu)))
        return nt.value, nu.value

    def evp_stress(self, dt, ndte, damping, ksub, icellt, indxti, indxtj, uvel, vvel, g, strength,
                   sig, diag, str8):
        ny, nx = uvel.shape
        self._ck(self.lib.cice_evp_stress(
            self.h, C.c_double(dt), ndte, int(damping), nx, ny, ksub, icellt, _i4(indxti), _i4(indxtj),
            _f8(uvel), _f8(vvel), _f8(g["dxt"]), _f8(g["dyt"]), _f8(g["dxhy"]), _f8(g["dyhx"]),
            _f8(g["cxp"]), _f8(g["cyp"]), _f8(g["cxm"]), _f8(g["cym"]), _f8(g["tarear"]),
            _f8(g["tinyarea"]), _f8(strength), *[_f8(sig[k]) for k in range(12)], _f8(diag["shear"]),
            _f8(diag["divu"]), _f8(diag["prs_sig"]), _f8(diag["rdg_conv"]), _f8(diag["rdg_shear"]),
            _f8(str8)))

    def evp_stepu(self, icellu, indxui, indxuj, aiu, str8, uocn, vocn, waterx, watery, forcex, forcey,
                  umassdtei, fm, uarear, strocnx, strocny, strintx, strinty, uvel, vvel):
        ny, nx = uvel.shape
        self._ck(self.lib.cice_evp_stepu(
            self.h, nx, ny, icellu, _i4(indxui), _i4(indxuj), _f8(aiu), _f8(str8), _f8(uocn), _f8(vocn),
            _f8(waterx), _f8(watery), _f8(forcex), _f8(forcey), _f8(umassdtei), _f8(fm), _f8(uarear),
            _f8(strocnx), _f8(strocny), _f8(strintx), _f8(strinty), _f8(uvel), _f8(vvel)))

    def halo_update(self, field, loc=1, kind=1, fill=0):
        """field: (nlev?, nblocks, ny, nx) float64 / float32 / int32, updated in place.  loc / kind: field location
        and type codes of ice_HaloUpdate (tripole fold); fill: value for ghost cells facing eliminated blocks."""
        n = self.nblocks * self.ny * self.nx
        nlev = field.size // n
        assert field.flags["C_CONTIGUOUS"]
        p = field.ctypes.data_as(C.c_void_p)
        if field.dtype == np.float64:
            self._ck(self.lib.cice_halo_update_ex_r8(self.h, p, nlev, loc, kind, C.c_double(fill)))
        elif field.dtype == np.float32:
            self._ck(self.lib.cice_halo_update_ex_r4(self.h, p, nlev, loc, kind, C.c_float(fill)))
        else:
            assert field.dtype == np.int32
            self._ck(self.lib.cice_halo_update_ex_i4(self.h, p, nlev, loc, kind, C.c_int32(int(fill))))

    def halo_update_blocked(self, field, loc=1, kind=1, fill=0):
        """The same for a field in the reference's own array layout (nblocks, nz, ny, nx) -- block outermost, what the
        Fortran boundary module hands over (cice_halo_update_blocked_*): only the frame of each block travels."""
        nz = field.size // (self.nblocks * self.ny * self.nx)
        assert field.flags["C_CONTIGUOUS"] and field.shape[0] == self.nblocks
        p = field.ctypes.data_as(C.c_void_p)
        if field.dtype == np.float64:
            self._ck(self.lib.cice_halo_update_blocked_r8(self.h, p, nz, loc, kind, C.c_double(fill)))
        elif field.dtype == np.float32:
            self._ck(self.lib.cice_halo_update_blocked_r4(self.h, p, nz, loc, kind, C.c_float(fill)))
        else:
            assert field.dtype == np.int32
            self._ck(self.lib.cice_halo_update_blocked_i4(self.h, p, nz, loc, kind, C.c_int32(int(fill))))

    def halo_update_strided(self, section, loc=1, kind=1, fill=0):
        """The same for a SECTION of a 4-d module array (cice_halo_update_strided_r8): a float64 view
        (nblocks, nz2, nz1, ny, nx) whose horizontal planes are whole and whose levels and blocks are strided, e.g.
        trcrn[:, :, 0:ntrcr] of an array (nblocks, ncat, max_ntrcr, ny, nx).  Updated in place; nothing outside the
        section is touched."""
        assert section.dtype == np.float64 and section.ndim == 5
        nb, nz2, nz1, ny, nx = section.shape
        assert (nb, ny, nx) == (self.nblocks, self.ny, self.nx)
        sb, s2, s1, sy, sx = (s // 8 for s in section.strides)
        assert (sy, sx) == (nx, 1) and all(s % 8 == 0 for s in section.strides), "the horizontal planes must be whole"
        self._ck(self.lib.cice_halo_update_strided_r8(self.h, C.c_void_p(section.ctypes.data), nz1, C.c_longlong(s1), nz2,
                                                      C.c_longlong(s2), C.c_longlong(sb), loc, kind, C.c_double(fill)))

    def halo_update_resident(self, field, loc=1, kind=1, fill=0):
        """The same on a field kept in device memory: upload once, update through cice_halo_update_dev_r8/_i4
        (all levels in one message per neighbour, no staging, no allocation per call), download.  With a location,
        kind or fill value other than the defaults: cice_halo_update_dev_ex_r8 (float64 only)."""
        n = self.nblocks * self.ny * self.nx
        nlev = field.size // n
        plain = (loc, kind, fill) == (1, 1, 0)
        if not plain and field.dtype != np.float64:
            raise CiceError("halo_update_resident: location / kind / fill on a resident field are float64 only")
        dev = C.c_void_p()
        self._ck(self.lib.cice_device_alloc(self.h, C.c_size_t(field.nbytes), C.byref(dev)))
        try:
            self._ck(self.lib.cice_device_copy(self.h, dev, _p(field), C.c_size_t(field.nbytes), 1))
            if plain:
                fn = self.lib.cice_halo_update_dev_r8 if field.dtype == np.float64 else self.lib.cice_halo_update_dev_i4
                self._ck(fn(self.h, dev, nlev))
            else:
                self._ck(self.lib.cice_halo_update_dev_ex_r8(self.h, dev, nlev, loc, kind, C.c_double(fill)))
            self._ck(self.lib.cice_device_copy(self.h, _p(field), dev, C.c_size_t(field.nbytes), 0))
        finally:
            self._ck(self.lib.cice_device_free(self.h, dev))

    # ---- thermodynamics ----------------------------------------------------------
    def thermo_init(self, heat_capacity=True, calc_Tsfc=True, conduct="MU71", ustar_min=0.05,
                    tr_iage=True, nt_Tsfc=1, nt_iage=2):
        cfg = ThermoConfig(int(heat_capacity), int(calc_Tsfc), 0 if conduct == "MU71" else 1, ustar_min,
                           int(tr_iage), nt_Tsfc, nt_iage)
        salin = np.zeros(NILYR + 1); tmlt = np.zeros(NILYR + 1)
        self._ck(self.lib.cice_thermo_init(self.h, C.byref(cfg), _f8(salin), _f8(tmlt)))
        return salin, tmlt

    def thermo_vertical(self, dt, icells, indxi, indxj, a, yday=1.0):
        ny, nx = a["aicen"].shape
        ls = C.c_int32(0); istop = C.c_int32(0); jstop = C.c_int32(0)
        self._ck(self.lib.cice_thermo_vertical(
            self.h, nx, ny, C.c_double(dt), icells, _i4(indxi), _i4(indxj),
            *[_f8(a[k]) for k in THERMO_ARGS], C.c_double(yday), C.byref(ls), C.byref(istop),
            C.byref(jstop)))
        return ls.value, istop.value, jstop.value

    def thermo_set_option(self, key, value):
        self._ck(self.lib.cice_thermo_set_option(self.h, key.encode(), int(value)))

    def thermo_batch_alloc(self, nx, ny, nblocks):
        self._ck(self.lib.cice_thermo_batch_alloc(self.h, nx, ny, nblocks))

    @staticmethod
    def _thermo_fields(a, outputs=True):
        f = ThermoFields()
        for n, _t in ThermoFields._fields_:
            setattr(f, n, _f8(a[n]) if n in a else None)
        return f

    def host_register(self, arr):
        """Page-lock a numpy array that will be passed to evp()/thermo entries repeatedly."""
        self._ck(self.lib.cice_host_register(self.h, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)))

    def host_unregister_all(self):
        """Must precede the release of any array handed to host_register / evp_pin_fields."""
        self._ck(self.lib.cice_host_unregister_all(self.h))

    def thermo_batch_upload(self, a):
        f = self._thermo_fields(a)
        self._ck(self.lib.cice_thermo_batch_upload(self.h, C.byref(f)))

    def thermo_batch_step(self, dt, yday=1.0, timed=False):
        nupd = C.c_longlong(0); ms = C.c_float(0.0)
        st = [C.c_int32(0) for _ in range(5)]
        self._ck(self.lib.cice_thermo_batch_step(self.h, C.c_double(dt), C.c_double(yday), C.byref(nupd),
                                                 *[C.byref(x) for x in st],
                                                 C.byref(ms) if timed else None))
        return dict(n_updates=nupd.value, l_stop=st[0].value, istop=st[1].value, jstop=st[2].value,
                    nstop=st[3].value, bstop=st[4].value, ms=ms.value)

    def thermo_batch_download(self, a):
        f = self._thermo_fields(a)
        self._ck(self.lib.cice_thermo_batch_download(self.h, C.byref(f)))

    def thermo_batch_merge(self, percat, acc):
        """percat: aicen_init, strairxn, strairyn, Trefn, Qrefn ((nb,ncat,ny,nx)); acc: dict keyed by
        MERGE_ORDER ((nb,ny,nx)), updated in place (merge_fluxes for every category)."""
        f = MergeFields()
        for n in ("aicen_init", "strairxn", "strairyn", "Trefn", "Qrefn"):
            setattr(f, n, _f8(percat[n]))
        for k, n in enumerate(MERGE_ORDER):
            f.acc[k] = acc[n].ctypes.data
            assert acc[n].dtype == np.float64 and acc[n].flags["C_CONTIGUOUS"]
        self._ck(self.lib.cice_thermo_batch_merge(self.h, C.byref(f)))

    # ---- horizontal transport --------------------------------------------------
    def transport_init(self, grid, ntrcr=2, trcr_depend=(0, 1)):
        """grid: HTN, HTE, dxt, dyt, dxu, dyu, tarear, hm as (nblocks, ny, nx) arrays; tracer set as in ice_init.F90:848."""
        cfg = TransportConfig()
        cfg.ntrcr = ntrcr
        for k, d in enumerate(trcr_depend):
            cfg.trcr_depend[k] = d
        g = TransportGrid()
        self._tgrid = {n: np.ascontiguousarray(grid[n], np.float64) for n, _t in TransportGrid._fields_}
        for n in self._tgrid:
            setattr(g, n, _f8(self._tgrid[n]))
        self._ck(self.lib.cice_transport_init(self.h, C.byref(cfg), C.byref(g)))

    def transport_upwind_init(self, HTE, HTN, tarea, ntrcr=2, trcr_depend=(0, 1), nt_Tsfc=1):
        cfg = TransportConfig()
        cfg.ntrcr = ntrcr
        for k, d in enumerate(trcr_depend):
            cfg.trcr_depend[k] = d
        self._ck(self.lib.cice_transport_upwind_init(self.h, C.byref(cfg), C.c_int(nt_Tsfc), _f8(HTE), _f8(HTN), _f8(tarea)))

    def transport_upwind(self, dt, s):
        """advection = 'upwind' on the arrays of transport_remap, updated in place"""
        f = TransportFields()
        for n, _t in TransportFields._fields_:
            setattr(f, n, _f8(s[n]))
        self._ck(self.lib.cice_transport_upwind(self.h, C.c_double(dt), C.byref(f)))

    def transport_remap(self, dt, s):
        """s: aice0, uvel, vvel (nb,ny,nx); aicen, vicen, vsnon (nb,ncat,ny,nx); trcrn (nb,ncat,5,ny,nx); eicen
        (nb,ncat*nilyr,ny,nx); esnon (nb,ncat*nslyr,ny,nx); state updated in place.  Returns (l_stop, istop, jstop)."""
        f = TransportFields()
        for n, _t in TransportFields._fields_:
            setattr(f, n, _f8(s[n]))
        st = [C.c_int32(0) for _ in range(3)]
        if getattr(self, "_ridge_mode", 0) == 2:
            self._handover = s   # keep the arrays alive: a deferred download lands in them (ridge_chain)
        self._ck(self.lib.cice_transport_remap(self.h, C.c_double(dt), C.byref(f), *[C.byref(x) for x in st]))
        return tuple(x.value for x in st)

    def ridge_chain(self, mode):
        """cice_ridge_chain: 0 off; 1: a step_ridge that follows a transport_remap and is given the SAME seven state
        arrays (aice0, aicen, trcrn, vicen, vsnon, eicen, esnon) takes the state from the transport's device buffers
        instead of uploading it; 2: as 1, and such a transport_remap leaves its result on the device -- the host arrays
        receive the state from step_ridge, from any other call on this context, or from transport_download_state()."""
        self._ck(self.lib.cice_ridge_chain(self.h, int(mode)))
        self._ridge_mode = int(mode)
        self._handover = None

    def ridge_chain_time(self, enable=True):
        """cice_ridge_chain_time: switch the event timing of the hand-over kernel on / off; the time (ms) of the last
        timed one"""
        ms = C.c_float(0.0)
        self._ck(self.lib.cice_ridge_chain_time(self.h, int(enable), C.byref(ms)))
        return ms.value

    def transport_download_state(self):
        """cice_transport_download_state: a transport result whose download was deferred (ridge_chain(2)) goes to the
        arrays that transport_remap call was given, and the hand-over ends; nothing happens if none is pending."""
        self._ck(self.lib.cice_transport_download_state(self.h))

    def transport_chain(self, s):
        """cice_transport_chain: s = the arrays the following transport_remap calls will be given (None ends the chain).
        Every evp(dt, ...) then prefetches the transport's state while it subcycles; a transport_remap that follows it with
        these arrays (and the uvel, vvel, aicen, vicen ARRAYS evp was given) uploads nothing."""
        if s is None:
            self._ck(self.lib.cice_transport_chain(self.h, None))
            self._chain = None
            return
        f = TransportFields()
        for n, _t in TransportFields._fields_:
            setattr(f, n, _f8(s[n]))
        self._chain = s          # keep the arrays alive: the library remembers their addresses
        self._ck(self.lib.cice_transport_chain(self.h, C.byref(f)))

    def transport_debug(self, stop_stage=0, which=-1):
        cnt = C.c_longlong(0)
        self._ck(self.lib.cice_transport_debug(self.h, stop_stage, which, None, C.byref(cnt)))
        if which < 0:
            return None
        out = np.zeros(cnt.value)
        self._ck(self.lib.cice_transport_debug(self.h, stop_stage, which, _f8(out), C.byref(cnt)))
        return out

    ATMO_OUT = ("strx", "stry", "Tref", "Qref", "delt", "delq", "lhcoef", "shcoef")

    def atmo_boundary_layer(self, sfctype, icells, indxi, indxj, a, calc_strair=True, strx=None, stry=None):
        """cice_atmo_boundary_layer (source/ice_atmo.F90:56).  a: Tsf, potT, uatm, vatm, wind, zlvl, Qa, rhoa (ny, nx);
        returns the eight outputs (strx, stry keep the given values when calc_strair is false)."""
        ny, nx = a["Tsf"].shape
        o = {k: np.zeros((ny, nx)) for k in self.ATMO_OUT}
        if strx is not None:
            o["strx"][...] = strx; o["stry"][...] = stry
        ins = [np.ascontiguousarray(a[k], np.float64) for k in ("Tsf", "potT", "uatm", "vatm", "wind", "zlvl", "Qa", "rhoa")]
        self._ck(self.lib.cice_atmo_boundary_layer(
            self.h, nx, ny, 0 if sfctype == "ice" else 1, icells, _i4(indxi), _i4(indxj), *[_f8(x) for x in ins],
            int(calc_strair), *[_f8(o[k]) for k in self.ATMO_OUT]))
        return o

    def step_therm1(self, dt, yday, state, fz, percat, acc, atm=None):
        """cice_step_therm1: one upload, frzmlt_bottom_lateral + thermo_vertical for every category + merge_fluxes on
        the device, one download.  state: thermo_batch_upload's dict (fbot/Tbot not needed); fz: aice, frzmlt, sst,
        Tf, strocnxT, strocnyT (+ optional outputs Tbot, fbot, rside), (nb,ny,nx); percat / acc as thermo_batch_merge
        (percat['aicen_init'] optional).  atm (cice_step_therm1_abl): uatm, vatm, wind, zlvl (+ strax, stray and
        calc_strair=False) -- atmo_boundary_layer runs on the device too, state's lhcoef/shcoef and percat's
        strairxn/strairyn/Trefn/Qrefn are not read; arrays found in atm under those six names are filled."""
        f = self._thermo_fields(state)
        z = FrzmltFields()
        for n, _t in FrzmltFields._fields_:
            setattr(z, n, _f8(fz[n]) if n in fz else None)
        m = MergeFields()
        for n in ("aicen_init", "strairxn", "strairyn", "Trefn", "Qrefn"):
            setattr(m, n, _f8(percat[n]) if n in percat else None)
        for k, n in enumerate(MERGE_ORDER):
            m.acc[k] = acc[n].ctypes.data
            assert acc[n].dtype == np.float64 and acc[n].flags["C_CONTIGUOUS"]
        nupd = C.c_longlong(0)
        st = [C.c_int32(0) for _ in range(5)]
        if atm is None:
            self._ck(self.lib.cice_step_therm1(self.h, C.c_double(dt), C.c_double(yday), C.byref(f), C.byref(z),
                                               C.byref(m), C.byref(nupd), *[C.byref(x) for x in st]))
        else:
            af = AtmoFields()
            for n, t in AtmoFields._fields_:
                if n == "calc_strair":
                    af.calc_strair = int(atm.get("calc_strair", True))
                else:
                    setattr(af, n, _f8(atm[n]) if n in atm else None)
            self._ck(self.lib.cice_step_therm1_abl(self.h, C.c_double(dt), C.c_double(yday), C.byref(f), C.byref(z),
                                                   C.byref(m), C.byref(af), C.byref(nupd), *[C.byref(x) for x in st]))
        return dict(n_updates=nupd.value, l_stop=st[0].value, istop=st[1].value, jstop=st[2].value,
                    nstop=st[3].value, bstop=st[4].value)

    def frzmlt_bottom_lateral(self, ilo, ihi, jlo, jhi, dt, aice, frzmlt, eicen, esnon, sst, Tf,
                              strocnxT, strocnyT):
        ny, nx = aice.shape
        Tbot = np.zeros((ny, nx)); fbot = np.zeros((ny, nx)); rside = np.zeros((ny, nx))
        self._ck(self.lib.cice_frzmlt_bottom_lateral(
            self.h, nx, ny, ilo, ihi, jlo, jhi, C.c_double(dt), _f8(aice), _f8(frzmlt), _f8(eicen),
            _f8(esnon), _f8(sst), _f8(Tf), _f8(strocnxT), _f8(strocnyT), _f8(Tbot), _f8(fbot),
            _f8(rside)))
        return Tbot, fbot, rside

    # ---- thermodynamic changes of the thickness distribution (ice_therm_itd) -----
    def itd_init(self, hin_max, ntrcr=1, trcr_depend=(0,), nt_Tsfc=1, nt_iage=0, nt_alvl=0, nt_vlvl=0, tr_iage=False,
                 tr_lvl=False, update_ocn_f=True, hi_min=0.01):
        """cice_itd_init: the module variables linear_itd / add_new_ice / lateral_melt read, after init_itd."""
        cfg = ItdConfig()
        cfg.ntrcr = ntrcr
        for k, d in enumerate(trcr_depend):
            cfg.trcr_depend[k] = d
        cfg.nt_Tsfc, cfg.nt_iage, cfg.nt_alvl, cfg.nt_vlvl = nt_Tsfc, nt_iage, nt_alvl, nt_vlvl
        cfg.tr_iage, cfg.tr_lvl, cfg.update_ocn_f = int(tr_iage), int(tr_lvl), int(update_ocn_f)
        for k in range(NCAT + 1):
            cfg.hin_max[k] = float(hin_max[k])
        cfg.hi_min = hi_min
        self._itd = (ntrcr, np.ascontiguousarray(trcr_depend, np.int32))
        self._ck(self.lib.cice_itd_init(self.h, C.byref(cfg)))

    def linear_itd(self, icells, indxi, indxj, a):
        """cice_linear_itd on one block.  a: aicen_init, vicen_init, aicen, vicen, vsnon (ncat,ny,nx), trcrn (ncat,5,ny,nx),
        eicen (ncat*nilyr,ny,nx), esnon (ncat*nslyr,ny,nx), aice, aice0 (ny,nx); updated in place.
        Returns (l_stop, istop, jstop, cells not remapped)."""
        ny, nx = a["aice"].shape
        ntr, dep = self._itd
        st = [C.c_int32(0) for _ in range(3)]
        nn = C.c_longlong(0)
        self._ck(self.lib.cice_linear_itd(
            self.h, nx, ny, icells, _i4(indxi), _i4(indxj), ntr, _i4(dep),
            *[_f8(a[k]) for k in ("aicen_init", "vicen_init", "aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "aice",
                                  "aice0")], *[C.byref(x) for x in st], C.byref(nn)))
        return st[0].value, st[1].value, st[2].value, nn.value

    def add_new_ice(self, icells, indxi, indxj, dt, yday, a):
        """cice_add_new_ice on one block.  a: tmask (int32), aicen, trcrn, vicen, eicen, aice0, aice, frzmlt, frazil,
        frz_onset, fresh, fsalt, Tf; updated in place.  Returns (l_stop, istop, jstop)."""
        ny, nx = a["aice"].shape
        st = [C.c_int32(0) for _ in range(3)]
        self._ck(self.lib.cice_add_new_ice(
            self.h, nx, ny, self._itd[0], icells, _i4(indxi), _i4(indxj), _i4(a["tmask"]), C.c_double(dt),
            *[_f8(a[k]) for k in ("aicen", "trcrn", "vicen", "eicen", "aice0", "aice", "frzmlt", "frazil", "frz_onset")],
            C.c_double(yday), _f8(a["fresh"]), _f8(a["fsalt"]), _f8(a["Tf"]), *[C.byref(x) for x in st]))
        return tuple(x.value for x in st)

    def lateral_melt(self, ilo, ihi, jlo, jhi, dt, a):
        """cice_lateral_melt on one block.  a: fresh, fsalt, fhocn, rside, meltl, aicen, vicen, vsnon, eicen, esnon."""
        ny, nx = a["rside"].shape
        self._ck(self.lib.cice_lateral_melt(
            self.h, nx, ny, ilo, ihi, jlo, jhi, C.c_double(dt),
            *[_f8(a[k]) for k in ("fresh", "fsalt", "fhocn", "rside", "meltl", "aicen", "vicen", "vsnon", "eicen", "esnon")]))

    def shift_ice(self, icells, indxi, indxj, a):
        """cice_shift_ice on one block.  a: aicen, trcrn, vicen, vsnon, eicen, esnon and hicen, donor (int32), daice, dvice
        as (ncat, icells).  Returns (l_stop, istop, jstop)."""
        ny, nx = a["aicen"].shape[-2:]
        ntr, dep = self._itd
        st = [C.c_int32(0) for _ in range(3)]
        self._ck(self.lib.cice_shift_ice(
            self.h, nx, ny, _i4(indxi), _i4(indxj), icells, ntr, _i4(dep),
            *[_f8(a[k]) for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "hicen")], _i4(a["donor"]),
            _f8(a["daice"]), _f8(a["dvice"]), *[C.byref(x) for x in st]))
        return tuple(x.value for x in st)

    def step_therm2_itd(self, dt, yday, a, kitd=1, state_resident=False):
        """cice_step_therm2_itd on the batch (thermo_batch_alloc).  a: the arrays of synth.therm2_state ((nb, ...));
        aicen_init may be missing with a resident state.  Returns dict(l_stop, istop, jstop, bstop, stage)."""
        f = Therm2Fields()
        f.ncat, f.kitd, f.state_resident = NCAT, int(kitd), int(state_resident)
        for n in THERM2_PTRS:
            setattr(f, n, (_i4(a[n]) if n == "tmask" else _f8(a[n])) if n in a else None)
        st = [C.c_int32(0) for _ in range(5)]
        self._ck(self.lib.cice_step_therm2_itd(self.h, C.c_double(dt), C.c_double(yday), C.byref(f),
                                               *[C.byref(x) for x in st]))
        return dict(zip(("l_stop", "istop", "jstop", "bstop", "stage"), (x.value for x in st)))

    # ---- the second half of step_therm2: cleanup_itd, bound_state, aggregate ------
    def cleanup_itd(self, ilo, ihi, jlo, jhi, dt, a, limit_aice=True, heat_capacity=True, fluxes=("fresh", "fsalt", "fhocn")):
        """cice_cleanup_itd on one block.  a: aicen, vicen, vsnon (ncat,ny,nx), trcrn (ncat,5,ny,nx), eicen, esnon, aice0,
        aice and the fluxes named in `fluxes` (the others are absent optionals); updated in place.
        Returns (l_stop, istop, jstop)."""
        ny, nx = a["aice"].shape
        ntr, dep = self._itd
        st = [C.c_int32(0) for _ in range(3)]
        self._ck(self.lib.cice_cleanup_itd(
            self.h, nx, ny, ilo, ihi, jlo, jhi, C.c_double(dt), ntr,
            *[_f8(a[k]) for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "aice0", "aice")], _i4(dep),
            *[_f8(a[k]) if k in fluxes else None for k in ("fresh", "fsalt", "fhocn")], int(heat_capacity),
            *[C.byref(x) for x in st], int(limit_aice)))
        return tuple(x.value for x in st)

    def aggregate(self, a):
        """cice_aggregate on one block.  a: the state and tmask (int32) in; aice, trcr (5,ny,nx), vice, vsno, eice, esno,
        aice0 out."""
        ny, nx = a["aice"].shape
        ntr, dep = self._itd
        self._ck(self.lib.cice_aggregate(
            self.h, nx, ny, *[_f8(a[k]) for k in ("aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "aice", "trcr", "vice",
                                                  "vsno", "eice", "esno", "aice0")], _i4(a["tmask"]), ntr, _i4(dep)))

    def step_therm2_cleanup(self, dt, a, state_resident=False, bound=False):
        """cice_step_therm2_cleanup on the batch (thermo_batch_alloc).  a: the arrays of CLEANUP_PTRS ((nb, ...)).
        Returns dict(l_stop, istop, jstop, bstop, stage)."""
        f = Therm2CleanupFields()
        f.ncat, f.state_resident, f.bound = NCAT, int(state_resident), int(bound)
        for n in CLEANUP_PTRS:
            setattr(f, n, _i4(a[n]) if n == "tmask" else _f8(a[n]))
        st = [C.c_int32(0) for _ in range(5)]
        self._ck(self.lib.cice_step_therm2_cleanup(self.h, C.c_double(dt), C.byref(f), *[C.byref(x) for x in st]))
        return dict(zip(("l_stop", "istop", "jstop", "bstop", "stage"), (x.value for x in st)))

    def therm2_cleanup_times(self, enable=True):
        """cice_therm2_cleanup_times: switch the event timing on / off; the times (ms) of the last timed call by CLEANUP_TIMES"""
        ms = (C.c_float * len(CLEANUP_TIMES))()
        self._ck(self.lib.cice_therm2_cleanup_times(self.h, int(enable), ms))
        return dict(zip(CLEANUP_TIMES, ms))

    # ---- mechanical redistribution (ice_mechred: ridge_ice) ------------------------
    RIDGE_OPTIONALS = ("dardg1dt", "dardg2dt", "dvirdgdt", "opening", "fresh", "fhocn")

    def ridge_init(self, krdg_partic=1, krdg_redist=1, mu_rdg=4.0):
        """cice_ridge_init: the namelist's ridging parameters (after itd_init, which gives tracers, tr_lvl, hin_max).
        krdg_redist = 0 raises CiceError with code CICE_EUNSUPPORTED."""
        self._ck(self.lib.cice_ridge_init(self.h, int(krdg_partic), int(krdg_redist), C.c_double(mu_rdg)))

    def ridge_ice(self, icells, indxi, indxj, dt, a, optionals=RIDGE_OPTIONALS):
        """cice_ridge_ice on one block.  a: rdg_conv, rdg_shear, aice0 (ny,nx), aicen, vicen, vsnon (ncat,ny,nx), trcrn
        (ncat,5,ny,nx), eicen, esnon and the arrays named in `optionals` (the others are absent optionals); updated in
        place.  Returns (l_stop, istop, jstop, niter)."""
        ny, nx = a["aice0"].shape
        ntr, dep = self._itd
        st = [C.c_int32(0) for _ in range(4)]
        self._ck(self.lib.cice_ridge_ice(
            self.h, nx, ny, C.c_double(dt), ntr, icells, _i4(indxi), _i4(indxj),
            *[_f8(a[k]) for k in ("rdg_conv", "rdg_shear", "aicen", "trcrn", "vicen", "vsnon", "eicen", "esnon", "aice0")],
            _i4(dep), *[C.byref(x) for x in st[:3]],
            *[_f8(a[k]) if k in optionals else None for k in self.RIDGE_OPTIONALS], C.byref(st[3])))
        return tuple(x.value for x in st)

    def step_ridge(self, dt, a, bound=False):
        """cice_step_ridge on the batch (thermo_batch_alloc).  a: the arrays of RIDGE_PTRS ((nb, ...)).
        Returns dict(l_stop, istop, jstop, bstop, stage)."""
        f = RidgeFields()
        f.ncat, f.bound = NCAT, int(bound)
        for n in RIDGE_PTRS:
            setattr(f, n, _i4(a[n]) if n == "tmask" else _f8(a[n]))
        st = [C.c_int32(0) for _ in range(5)]
        self._ck(self.lib.cice_step_ridge(self.h, C.c_double(dt), C.byref(f), *[C.byref(x) for x in st]))
        return dict(zip(("l_stop", "istop", "jstop", "bstop", "stage"), (x.value for x in st)))

    def ridge_times(self, enable=True):
        """cice_ridge_times: switch the event timing on / off; the times (ms) of the last timed call by RIDGE_TIMES"""
        ms = (C.c_float * len(RIDGE_TIMES))()
        self._ck(self.lib.cice_ridge_times(self.h, int(enable), ms))
        return dict(zip(RIDGE_TIMES, ms))

    # ---- shortwave radiation, shortwave = 'default' (ice_shortwave: shortwave_ccsm3) ---------
    SHORTWAVE_OUT = ("alvdrn", "alidrn", "alvdfn", "alidfn", "fswsfc", "fswint", "fswthru", "Iswabs", "albin", "albsn")

    def shortwave_init(self, shortwave="default", albedo_type="default", albicev=0.78, albicei=0.36, albsnowv=0.98,
                       albsnowi=0.70, ahmax=0.3, albocn=0.06, dT_mlt=1.0, dalb_mlt=-0.075, snowpatch=0.02,
                       awtvdr=0.00318, awtidr=0.00182, awtvdf=0.63282, awtidf=0.36218):
        """cice_shortwave_init (after thermo_init, which gives heat_capacity, calc_Tsfc, nt_Tsfc).  The defaults are the
        reference's namelist defaults and the stand-alone build's parameters.  shortwave='dEdd' raises CiceError with
        code CICE_EUNSUPPORTED."""
        cfg = ShortwaveConfig({"default": 0, "dEdd": 1}[shortwave], {"default": 0, "constant": 1}[albedo_type], albicev,
                              albicei, albsnowv, albsnowi, ahmax, albocn, dT_mlt, dalb_mlt, snowpatch, awtvdr, awtidr,
                              awtvdf, awtidf)
        self._ck(self.lib.cice_shortwave_init(self.h, C.byref(cfg)))

    def shortwave_ccsm3(self, icells, indxi, indxj, a, ocn_albedo=None):
        """cice_shortwave_ccsm3 on one block and category.  a: aicen, vicen, vsnon, Tsfcn, swvdr, swvdf, swidr, swidf
        (ny,nx) in; the arrays of SHORTWAVE_OUT ((ny,nx), Iswabs (nilyr,ny,nx)) are written on the whole block.
        ocn_albedo: the -DAusCOM build's last argument, None = absent."""
        ny, nx = a["aicen"].shape
        self._ck(self.lib.cice_shortwave_ccsm3(
            self.h, nx, ny, icells, _i4(indxi), _i4(indxj),
            *[_f8(a[k]) for k in ("aicen", "vicen", "vsnon", "Tsfcn", "swvdr", "swvdf", "swidr", "swidf")],
            *[_f8(a[k]) for k in self.SHORTWAVE_OUT], _f8(ocn_albedo)))

    def step_radiation(self, a, state_resident=False):
        """cice_step_radiation on the batch (thermo_batch_alloc).  a: swvdr, swvdf, swidr, swidf (nb,ny,nx), the arrays of
        RADIATION_OUT, and -- unless state_resident -- aicen, trcrn, vicen, vsnon; optional ocn_albedo, coszen."""
        f = RadiationFields()
        f.ncat, f.state_resident = NCAT, int(state_resident)
        for n, _t in RadiationFields._fields_[2:]:
            setattr(f, n, _f8(a[n]) if a.get(n) is not None else None)
        self._ck(self.lib.cice_step_radiation(self.h, C.byref(f)))

    def prep_radiation(self, a, sw_resident=False):
        """cice_prep_radiation on the batch.  a: the arrays of PREP_RADIATION_PTRS; scale_factor, fswfac and the five
        shortwave arrays are updated in place (sw_resident: the device copies are scaled, the five are written only)."""
        f = PrepRadiationFields()
        f.ncat, f.sw_resident = NCAT, int(sw_resident)
        for n in PREP_RADIATION_PTRS:
            setattr(f, n, _f8(a[n]) if a.get(n) is not None else None)
        self._ck(self.lib.cice_prep_radiation(self.h, C.byref(f)))

    def radiation_chain(self, mode):
        """cice_radiation_chain: 0 off; 1: a step_therm1 that follows a step_radiation / prep_radiation and is given the
        SAME five arrays fswsfc, fswint, fswthrun, Sswabs, Iswabs those calls downloaded to uploads none of them."""
        self._ck(self.lib.cice_radiation_chain(self.h, int(mode)))

    def radiation_times(self, enable=True):
        """cice_radiation_times: switch the event timing on / off; (k_shortwave_ccsm3, k_prep_radiation) ms of the last
        timed calls"""
        ms = (C.c_float * 2)()
        self._ck(self.lib.cice_radiation_times(self.h, int(enable), ms))
        return tuple(ms)

    # ---- shortwave radiation, shortwave = 'dEdd' (ice_shortwave: shortwave_dEdd) --------------
    DEDD_IN = ("coszen", "aice", "vice", "vsno", "fs", "rhosnw", "rsnw", "fp", "hp", "swvdr", "swvdf", "swidr", "swidf")
    DEDD_OUT = ("alvdr", "alvdf", "alidr", "alidf", "fswsfc", "fswint", "fswthru", "Sswabs", "Iswabs", "albice", "albsno",
                "albpnd")

    def shortwave_dedd_init(self, R_ice=0.0, R_pnd=0.0, R_snw=0.0, awtvdr=0.00318, awtidr=0.00182, awtvdf=0.63282,
                            awtidf=0.36218, tr_pond=False):
        """cice_shortwave_dedd_init (after thermo_init).  The defaults are the reference's namelist defaults and the
        weights of ice_constants.  Independent of shortwave_init: a context may hold both schemes."""
        cfg = DeddConfig(R_ice, R_pnd, R_snw, awtvdr, awtidr, awtvdf, awtidf, int(tr_pond))
        self._ck(self.lib.cice_shortwave_dedd_init(self.h, C.byref(cfg)))

    def shortwave_dEdd(self, icells, indxi, indxj, a):
        """cice_shortwave_dEdd on one block and category.  a: the arrays of DEDD_IN ((ny,nx); rhosnw, rsnw (nslyr,ny,nx))
        in; the arrays of DEDD_OUT ((ny,nx), Sswabs (nslyr,ny,nx), Iswabs (nilyr,ny,nx)) are written on the whole block."""
        ny, nx = a["aice"].shape
        self._ck(self.lib.cice_shortwave_dEdd(self.h, nx, ny, icells, _i4(indxi), _i4(indxj),
                                              *[_f8(a[k]) for k in self.DEDD_IN], *[_f8(a[k]) for k in self.DEDD_OUT]))

    def step_radiation_dedd(self, a, state_resident=False):
        """cice_step_radiation_dedd on the batch (thermo_batch_alloc).  a: swvdr, swvdf, swidr, swidf, coszen (nb,ny,nx),
        the arrays of RADIATION_DEDD_OUT, under tr_pond apondn and hpondn, and -- unless state_resident -- aicen, trcrn,
        vicen, vsnon."""
        f = RadiationDeddFields()
        f.ncat, f.state_resident = NCAT, int(state_resident)
        for n, _t in RadiationDeddFields._fields_[2:]:
            setattr(f, n, _f8(a[n]) if a.get(n) is not None else None)
        self._ck(self.lib.cice_step_radiation_dedd(self.h, C.byref(f)))

    def dedd_times(self, enable=True):
        """cice_dedd_times: switch the event timing on / off; the device time (ms) of the last timed k_shortwave_dedd"""
        ms = (C.c_float * 1)()
        self._ck(self.lib.cice_dedd_times(self.h, int(enable), ms))
        return ms[0]

    # ---- coupling_prep: the mixed layer, the albedo merge, scale_fluxes --------------------------
    def coupling_init(self, scale_fluxes=True, oceanmixed_ice=True, atmbndy="default", albocn=0.06):
        """cice_coupling_init (after thermo_init).  scale_fluxes=False: what a reference compiled -DAusCOM does.
        atmbndy='constant' raises CiceError with code CICE_EUNSUPPORTED."""
        cfg = CouplingConfig(int(scale_fluxes), int(oceanmixed_ice), {"default": 0, "constant": 1}[atmbndy], albocn)
        self._ck(self.lib.cice_coupling_init(self.h, C.byref(cfg)))

    def coupling_prep(self, dt, a, state_resident=False, alb_resident=False, bound=False, nstreams=0, ncat=NCAT):
        """cice_coupling_prep on the batch (thermo_batch_alloc).  a: tmask (int32, (nb,ny,nx)) and the arrays of
        COUPLING_PTRS -- per-category ones (nb,ncat,ny,nx), 2-d fields (nb,ny,nx), albcnt (nstreams,nb,ny,nx); a missing
        key is a NULL pointer.  The fields of COUPLING_FLUXES, albcnt, sst and qdp are updated in place, those of
        COUPLING_OUT, COUPLING_MIX_OUT and COUPLING_MIX_OPT written."""
        f = CouplingFields()
        f.ncat, f.state_resident, f.alb_resident, f.bound, f.nstreams = ncat, int(state_resident), int(alb_resident), \
            int(bound), int(nstreams)
        f.tmask = _i4(a["tmask"]) if a.get("tmask") is not None else None
        for n in COUPLING_PTRS:
            setattr(f, n, _f8(a[n]) if a.get(n) is not None else None)
        self._ck(self.lib.cice_coupling_prep(self.h, C.c_double(dt), C.byref(f)))

    def coupling_times(self, enable=True):
        """cice_coupling_times: switch the event timing on / off; (k_ocean_mixed_layer, k_coupling_prep) ms of the last
        timed call"""
        ms = (C.c_float * 2)()
        self._ck(self.lib.cice_coupling_times(self.h, int(enable), ms))
        return tuple(ms)

    # ---- melt ponds and ice age: compute_ponds, increment_age behind step_therm1 -------------------
    def pond_init(self, nt_volpn=0):
        """cice_pond_init (after thermo_init, which supplies nt_Tsfc, tr_iage, nt_iage).  nt_volpn: the 1-based slot of the
        pond volume tracer; 0: no pond tracer (only the age part may be asked for)."""
        self._ck(self.lib.cice_pond_init(self.h, int(nt_volpn)))

    def compute_ponds(self, ilo, ihi, jlo, jhi, dt, a):
        """cice_compute_ponds on one block and category.  a: meltt, melts, frain, aicen, vicen, vsnon (ny,nx) in; trcrn
        (max_ntrcr,ny,nx), apondn, hpondn (ny,nx) updated in place on the cells with aicen > puny of ilo..ihi, jlo..jhi."""
        ny, nx = a["aicen"].shape
        self._ck(self.lib.cice_compute_ponds(self.h, nx, ny, ilo, ihi, jlo, jhi, C.c_double(dt),
                                             *[_f8(a[k]) for k in ("meltt", "melts", "frain", "aicen", "vicen", "vsnon",
                                                                   "trcrn", "apondn", "hpondn")]))

    def increment_age(self, dt, icells, indxi, indxj, iage):
        """cice_increment_age on one block and category: iage (ny,nx) + dt on the cells of the list, in place."""
        ny, nx = iage.shape
        self._ck(self.lib.cice_increment_age(self.h, nx, ny, C.c_double(dt), icells, _i4(indxi), _i4(indxj), _f8(iage)))

    def step_ponds(self, dt, a, state_resident=False, ponds=True, age=True, ncat=NCAT):
        """cice_step_ponds on the batch (thermo_batch_alloc).  a: the arrays of POND_PTRS -- frain (nb,ny,nx), trcrn
        (nb,ncat,max_ntrcr,ny,nx), the others (nb,ncat,ny,nx); a missing key is a NULL pointer.  apondn, hpondn and the
        planes nt_volpn, nt_iage of trcrn are updated in place; with state_resident aicen, vicen, vsnon, melttn, meltsn
        are not read (what the last step_therm1 left on the device is)."""
        f = PondFields()
        f.ncat, f.state_resident, f.ponds, f.age = ncat, int(state_resident), int(ponds), int(age)
        for n in POND_PTRS:
            setattr(f, n, _f8(a[n]) if a.get(n) is not None else None)
        self._ck(self.lib.cice_step_ponds(self.h, C.c_double(dt), C.byref(f)))

    def pond_times(self, enable=True):
        """cice_pond_times: switch the event timing on / off; the device time (ms) of the last timed k_pond_age"""
        ms = (C.c_float * 1)()
        self._ck(self.lib.cice_pond_times(self.h, int(enable), ms))
        return ms[0]

    def pond_chain(self, mode):
        """cice_pond_chain: 1: a step_radiation_dedd under tr_pond that is given the apondn, hpondn arrays the last
        step_ponds downloaded to reads the device copies instead of uploading them; 0 (the default): off."""
        self._ck(self.lib.cice_pond_chain(self.h, int(mode)))

    def therm2_itd_times(self, enable=True):
        """cice_therm2_itd_times: switch the event timing of the stage's kernels on / off; the times (ms) of the last timed call"""
        ms = (C.c_float * 4)()
        self._ck(self.lib.cice_therm2_itd_times(self.h, int(enable), ms))
        return tuple(ms)
