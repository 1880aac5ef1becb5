// k_shortwave_dedd and the host-side tuning of the ice optical properties (dedd.h).
#include "dedd.h"

#include <cmath>

#include "dedd_tables.h"

namespace cice {

namespace {

using namespace dedd_tab;

static_assert(NILYR >= 2 && NSLYR >= 1, "the layer structure of compute_dEdd: ssl + dl + lowest layer, one snow layer at least");

constexpr int klev = NSLYR + NILYR + 1;   // layers 0 .. klev
constexpr int klevp = klev + 1;           // interfaces 0 .. klevp
constexpr int kii = NSLYR + 1;            // the sea ice ssl

constexpr double c3 = 3.0, c1p5 = 1.5, p75 = 0.75, p01 = 0.01, Timelt = 0.0;
// compute_dEdd :2028-2033, :2305-2322 (data statements: run-time values in the reference, no folding across them)
constexpr double cp67 = 0.67, cp33 = 0.33, cp78 = 0.78, cp22 = 0.22, cp01 = 0.01;
constexpr double hs_ssl = 0.040, rhoi_snw = 917.0, fr_max = 1.00, fr_min = 0.80, hi_ssl = 0.050, kalg = 0.60;
constexpr double hpmin = 0.005, hp0 = 0.200;
// solution_dEdd :3054-3091, :3135-3144
constexpr double trmin = 0.001, refindx = 1.310, cp063 = 0.063, cp455 = 0.455;
constexpr int ngmax = 8;
constexpr double gauspt[ngmax] = {0.9894009, 0.9445750, 0.8656312, 0.7554044, 0.6178762, 0.4580168, 0.2816036, 0.0950125};
constexpr double gauswt[ngmax] = {0.0271525, 0.0622535, 0.0951585, 0.1246290, 0.1495960, 0.1691565, 0.1826034, 0.1894506};
// shortwave_dEdd_set_snow :3528-3537
constexpr double hsmin = 0.0001, hs0 = 0.0300, dT_mlt = 1.0, rsnw_fresh = 100.0, rsnw_nonmelt = 500.0, rsnw_sig = 250.0,
                 rsnw_melt = 1000.0;

CICE_HD inline double dmax(double a, double b) { return a > b ? a : b; }
CICE_HD inline double dmin(double a, double b) { return a < b ? a : b; }

// the statement functions of solution_dEdd (:3159-3167), parenthesised as written
CICE_HD inline double sf_alpha(double w, double uu, double gg, double e) {
  return p75 * w * uu * ((K::c1 + gg * (K::c1 - w)) / (K::c1 - e * e * uu * uu));
}
CICE_HD inline double sf_gamma(double w, double uu, double gg, double e) {
  return K::p5 * w * ((K::c1 + c3 * gg * (K::c1 - w) * uu * uu) / (K::c1 - e * e * uu * uu));
}
CICE_HD inline double sf_n(double uu, double et) { return ((uu + K::c1) * (uu + K::c1) / et) - ((uu - K::c1) * (uu - K::c1) * et); }
CICE_HD inline double sf_u(double w, double gg, double e) { return c1p5 * (K::c1 - w * gg) / e; }
CICE_HD inline double sf_el(double w, double gg) { return sqrt(c3 * (K::c1 - w) * (K::c1 - w * gg)); }
CICE_HD inline double sf_taus(double w, double f, double t) { return (K::c1 - w * f) * t; }
CICE_HD inline double sf_omgs(double w, double f) { return (K::c1 - f) * w / (K::c1 - w * f); }
CICE_HD inline double sf_asys(double gg, double f) { return (gg - f) / (K::c1 - f); }

// one (cell, category) of shortwave_dEdd: the inputs as the reference's routine has them
struct Col {
  double aice, vice, vsno, coszen, swvdr, swvdf, swidr, swidf, fs, fp, hp, rhosnw[NSLYR], rsnw[NSLYR];
};
struct ColOut {
  double alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, Sswabs[NSLYR], Iswabs[NILYR], albice, albsno, albpnd;
};
// what one compute_dEdd leaves for its cell before the weighting with the surface type's fraction
struct Pass {
  double avdr, avdf, aidr, aidf, fsfc, fint, fthru, Sabs[NSLYR], Iabs[NILYR];
};

// apparent optical properties of a layer
struct Layer {
  double rdir, rdif_a, rdif_b, tdir, tdif_a, tdif_b, trnlay;
};

// The Delta-Eddington solution of one layer (:3244-3390).  The layer index enters through above_fresnel (k < kfrsnl on a
// cell without pond: the unrefracted beam) and fresnel (k == kfrsnl).  Every exp is exp_libm with the reference's argument
// expression.  exp_libm restates glibc for |x| < 512; beyond that (thick snow in the third band: -ts/mu below -512) the
// true value is far below exp_min = exp(-10) and so is whatever the restatement's fallback returns for a large negative
// argument, so the word is exp_min either way.
CICE_HD inline Layer layer_solution(double tautot, double wtot, double gtot, double mu0, bool above_fresnel, bool fresnel,
                                    double exp_min) {
  Layer L;
  const double ftot = gtot * gtot;
  const double ts = sf_taus(wtot, ftot, tautot);
  const double ws = sf_omgs(wtot, ftot);
  const double gs = sf_asys(gtot, ftot);
  const double lm = sf_el(ws, gs);
  const double ue = sf_u(ws, gs, lm);
  double mu0n = sqrt(K::c1 - ((K::c1 - mu0 * mu0) / (refindx * refindx)));
  if (above_fresnel) mu0n = mu0;
  const double extins = dmax(exp_min, exp_libm(-lm * ts));
  const double ne = sf_n(ue, extins);
  double rdif_a = (ue + K::c1) * (ue - K::c1) * (K::c1 / extins - extins) / ne;
  double tdif_a = K::c4 * ue / ne;
  double trnlay = dmax(exp_min, exp_libm(-ts / (mu0n)));
  double alp = sf_alpha(ws, mu0n, gs, lm);
  double gam = sf_gamma(ws, mu0n, gs, lm);
  double apg = alp + gam;
  double amg = alp - gam;
  double rdir = amg * (tdif_a * trnlay - K::c1) + apg * rdif_a;
  double tdir = apg * tdif_a + (amg * rdif_a - (apg - K::c1)) * trnlay;
  // rdif, tdif again by gaussian integration over the direct solution
  double swt = K::c0, smr = K::c0, smt = K::c0;
#pragma unroll 1
  for (int ng = 0; ng < ngmax; ++ng) {
    const double mu = gauspt[ng];
    const double gwt = gauswt[ng];
    swt = swt + mu * gwt;
    const double trn = dmax(exp_min, exp_libm(-ts / (mu)));
    alp = sf_alpha(ws, mu, gs, lm);
    gam = sf_gamma(ws, mu, gs, lm);
    apg = alp + gam;
    amg = alp - gam;
    const double rdr = amg * (tdif_a * trn - K::c1) + apg * rdif_a;
    const double tdr = apg * tdif_a + (amg * rdif_a - (apg - K::c1)) * trn;
    smr = smr + mu * rdr * gwt;
    smt = smt + mu * tdr * gwt;
  }
  rdif_a = smr / swt;
  tdif_a = smt / swt;
  double rdif_b = rdif_a, tdif_b = tdif_a;   // homogeneous layer
  if (fresnel) {                            // the refracting boundary on top of this layer (:3338-3390)
    const double R1 = (mu0 - refindx * mu0n) / (mu0 + refindx * mu0n);
    const double R2 = (refindx * mu0 - mu0n) / (refindx * mu0 + mu0n);
    const double T1 = K::c2 * mu0 / (mu0 + refindx * mu0n);
    const double T2 = K::c2 * mu0 / (refindx * mu0 + mu0n);
    const double Rf_dir_a = K::p5 * (R1 * R1 + R2 * R2);
    const double Tf_dir_a = K::p5 * (T1 * T1 + T2 * T2) * refindx * mu0n / mu0;
    const double Rf_dif_a = cp063, Tf_dif_a = K::c1 - Rf_dif_a;
    const double Rf_dif_b = cp455, Tf_dif_b = K::c1 - Rf_dif_b;
    const double rintfc = K::c1 / (K::c1 - Rf_dif_b * rdif_a);
    tdir = Tf_dir_a * tdir + Tf_dir_a * rdir * Rf_dif_b * rintfc * tdif_a;
    rdir = Rf_dir_a + Tf_dir_a * rdir * rintfc * Tf_dif_b;
    rdif_a = Rf_dif_a + Tf_dif_a * rdif_a * rintfc * Tf_dif_b;
    rdif_b = rdif_b + tdif_b * Rf_dif_b * rintfc * tdif_a;
    tdif_a = Tf_dif_a * rintfc * tdif_a;
    tdif_b = tdif_b * rintfc * Tf_dif_b;
    trnlay = Tf_dir_a * trnlay;
  }
  L.rdir = rdir; L.rdif_a = rdif_a; L.rdif_b = rdif_b; L.tdir = tdir; L.tdif_a = tdif_a; L.tdif_b = tdif_b; L.trnlay = trnlay;
  return L;
}

// The solar beam transmission, total transmission, reflectivity to diffuse radiation from below and diffuse transmission
// at the interface under layer m from those at the interface above it (:3227-3235, :3411-3419)
CICE_HD inline void interface_below(const Layer& m, double trndir0, double trntdr0, double trndif0, double rdndif0,
                                    double& trndir, double& trntdr, double& trndif, double& rdndif) {
  trndir = trndir0 * m.trnlay;
  const double refkm1 = K::c1 / (K::c1 - rdndif0 * m.rdif_a);
  const double tdrrdir = trndir0 * m.rdir;
  const double tdndif = trntdr0 - trndir0;
  trntdr = trndir0 * m.tdir + (tdndif + tdrrdir * rdndif0) * refkm1 * m.tdif_a;
  rdndif = m.rdif_b + (m.tdif_b * rdndif0 * refkm1 * m.tdif_a);
  trndif = trndif0 * refkm1 * m.tdif_a;
}

// Snow optical properties of one snow layer and band by interpolation in the grain radius (:2459-2484).  The lookup is
// data-dependent per lane: two rows of three tables from read-only global memory (2.3 KB in all, resident in the vector
// L1 / L2) -- six loads per band against some thousand fp64 operations, so nothing is staged in the LDS.
CICE_HD inline void snow_iops(int ns, double fr, double rsnw, double rhosnw, double& ks, double& ws, double& gs) {
  const double x = fr * rsnw;
  double Qs;
  if (x < rsnw_tab[0]) {
    Qs = Qs_tab[ns]; ws = ws_tab[ns]; gs = gs_tab[ns];
  } else if (x >= rsnw_tab[nmbrad - 1]) {
    Qs = Qs_tab[(nmbrad - 1) * nspint + ns]; ws = ws_tab[(nmbrad - 1) * nspint + ns]; gs = gs_tab[(nmbrad - 1) * nspint + ns];
  } else {
    int nr = 1;                              // rsnw_tab[nr - 1] <= x < rsnw_tab[nr]
    while (nr < nmbrad - 1 && rsnw_tab[nr] <= x) ++nr;
    const double delr = (x - rsnw_tab[nr - 1]) / (rsnw_tab[nr] - rsnw_tab[nr - 1]);
    const int lo = (nr - 1) * nspint + ns, hi = nr * nspint + ns;
    Qs = Qs_tab[lo] * (K::c1 - delr) + Qs_tab[hi] * delr;
    ws = ws_tab[lo] * (K::c1 - delr) + ws_tab[hi] * delr;
    gs = gs_tab[lo] * (K::c1 - delr) + gs_tab[hi] * delr;
  }
  ks = Qs * ((rhosnw / rhoi_snw) * 3.0 / (4.0 * fr * rsnw * 1.0e-6));
}

// Element ns of a kernel argument's array by selection: a run-time index into the by-value argument would move the whole
// structure to scratch memory.
CICE_HD inline double pick(const double (&a)[3], int ns) { return ns == 0 ? a[0] : (ns == 1 ? a[1] : a[2]); }

// compute_dEdd (:1796-2903) for one cell and one surface type: 0 bare ice (air above), 1 snow, 2 pond
CICE_HD inline void compute_pass(const DeddParams& p, const Col& c, int srftyp, double hs, double hi, double fnidr, Pass& o) {
  o.avdr = o.avdf = o.aidr = o.aidf = o.fsfc = o.fint = o.fthru = K::c0;
#pragma unroll
  for (int k = 0; k < NSLYR; ++k) o.Sabs[k] = K::c0;
#pragma unroll
  for (int k = 0; k < NILYR; ++k) o.Iabs[k] = K::c0;
  const double wght2 = cp67 + (cp78 - cp67) * (K::c1 - fnidr), wght3 = cp33 + (cp22 - cp33) * (K::c1 - fnidr);
  const double mu0 = dmax(c.coszen, p01);
  // layer thicknesses: snow or pond above, sea ice below
  double dzs = K::c0, dzs_ssl = K::c0, fr = K::c0;
  if (srftyp == 1) {
    dzs_ssl = hs_ssl;
    dzs = hs / (double)NSLYR;
    dzs_ssl = dmin(dzs_ssl, dzs / K::c2);
    fr = fr_max * fnidr + fr_min * (K::c1 - fnidr);
  } else if (srftyp == 2) {
    dzs = c.hp / (double)(NSLYR + 1);
  }
  double dz_ssl = hi_ssl;
  const double dz = hi / (double)NILYR;
  if (hi < 1.5) dz_ssl = hi / 30.0;
  dz_ssl = dmin(dz_ssl, dz / K::c2);
  const double fsdl = (double)NILYR / (double)4;
  const bool transition = srftyp == 2 && hpmin <= c.hp && c.hp <= hp0;

#pragma unroll 1
  for (int ns = 0; ns < nspint; ++ns) {
    // downward sweep: interface k is the top of layer k
    double trndir[klevp + 1], trntdr[klevp + 1], trndif[klevp + 1], rdndif[klevp + 1];
    Layer L[klev + 1];
    trndir[0] = K::c1; trntdr[0] = K::c1; trndif[0] = K::c1; rdndif[0] = K::c0;
    double ks_s = K::c0, ws_s = K::c0, gs_s = K::c0;
#pragma unroll
    for (int k = 0; k <= klev; ++k) {
      if (k > 0) interface_below(L[k - 1], trndir[k - 1], trntdr[k - 1], trndif[k - 1], rdndif[k - 1], trndir[k], trntdr[k],
                                 trndif[k], rdndif[k]);
      // optical properties of layer k (:2431-2604)
      double tau, w0, g;
      if (k <= NSLYR) {
        if (srftyp == 0) {
          tau = K::c0; w0 = K::c0; g = K::c0;
        } else if (srftyp == 1) {
          // (the snow ssl and the rest of the top snow layer share the top layer's radius and density)
          if (k == 0 || k > 1) {
            const int ksnow = k > 1 ? k - 1 : 0;
            snow_iops(ns, fr, c.rsnw[ksnow], c.rhosnw[ksnow], ks_s, ws_s, gs_s);
          }
          tau = k == 0 ? ks_s * dzs_ssl : (k == 1 ? ks_s * (dzs - dzs_ssl) : ks_s * dzs);
          w0 = ws_s; g = gs_s;
        } else {
          tau = kw[ns] * dzs; w0 = ww[ns]; g = gw[ns];
        }
      } else if (srftyp <= 1) {
        if (k == klev) {                     // lowest layer, with algae in the visible
          double kabs = pick(p.ki_int, ns) * (K::c1 - pick(p.wi_int, ns));
          if (ns == 0) kabs = kabs + kalg * (0.50 / dz);
          const double sig = pick(p.ki_int, ns) * pick(p.wi_int, ns);
          tau = (kabs + sig) * dz; w0 = (sig / (sig + kabs)); g = pick(p.gi_int, ns);
        } else if (k == kii) {
          tau = pick(p.ki_ssl, ns) * dz_ssl; w0 = pick(p.wi_ssl, ns); g = pick(p.gi_ssl, ns);
        } else if (k == kii + 1) {
          tau = pick(p.ki_dl, ns) * (dz - dz_ssl) * fsdl; w0 = pick(p.wi_dl, ns); g = pick(p.gi_dl, ns);
        } else {
          tau = pick(p.ki_int, ns) * dz; w0 = pick(p.wi_int, ns); g = pick(p.gi_int, ns);
        }
      } else if (!transition) {
        if (k == kii) {
          tau = pick(p.ki_p_ssl, ns) * dz_ssl; w0 = pick(p.wi_p_ssl, ns); g = pick(p.gi_p_ssl, ns);
        } else if (k == kii + 1) {
          tau = pick(p.ki_p_int, ns) * (dz - dz_ssl); w0 = pick(p.wi_p_int, ns); g = pick(p.gi_p_int, ns);
        } else {
          tau = pick(p.ki_p_int, ns) * dz; w0 = pick(p.wi_p_int, ns); g = pick(p.gi_p_int, ns);
        }
      } else {                               // shallow pond: between bare and ponded ice (:2572-2602)
        double sig_i, sig_p, kab, thick;
        if (k == kii) {
          sig_i = pick(p.ki_ssl, ns) * pick(p.wi_ssl, ns); sig_p = pick(p.ki_p_ssl, ns) * pick(p.wi_p_ssl, ns);
          kab = pick(p.ki_p_ssl, ns) * (K::c1 - pick(p.wi_p_ssl, ns)); thick = dz_ssl;
        } else if (k == kii + 1) {
          sig_i = pick(p.ki_dl, ns) * pick(p.wi_dl, ns) * fsdl; sig_p = pick(p.ki_p_int, ns) * pick(p.wi_p_int, ns);
          kab = pick(p.ki_p_int, ns) * (K::c1 - pick(p.wi_p_int, ns)); thick = dz - dz_ssl;
        } else {
          sig_i = pick(p.ki_int, ns) * pick(p.wi_int, ns); sig_p = pick(p.ki_p_int, ns) * pick(p.wi_p_int, ns);
          kab = pick(p.ki_p_int, ns) * (K::c1 - pick(p.wi_p_int, ns)); thick = dz;
        }
        const double sig = sig_i + (sig_p - sig_i) * (c.hp / hp0);
        const double kext = sig + kab;
        tau = kext * thick; w0 = sig / kext; g = pick(p.gi_p_int, ns);
      }
      // a layer the beam does not reach with more than trmin is left at zero (:3240): data-dependent, and it changes bits
      if (trntdr[k] > trmin) {
        const int kfrsnl = NSLYR + 2;
        L[k] = layer_solution(tau, w0, g, mu0, srftyp < 2 && k < kfrsnl, srftyp < 2 ? k == kfrsnl : k == 0, p.exp_min);
      } else {
        L[k].rdir = L[k].rdif_a = L[k].rdif_b = L[k].tdir = L[k].tdif_a = L[k].tdif_b = L[k].trnlay = K::c0;
      }
    }
    interface_below(L[klev], trndir[klev], trntdr[klev], trndif[klev], rdndif[klev], trndir[klevp], trntdr[klevp],
                    trndif[klevp], rdndif[klevp]);
    // upward sweep from the ocean (:3433-3455) with the interface fluxes (:2649-2670) on the way: F[k] is the net downward
    // flux through interface k for this band's incident direct and diffuse radiation
    const double swdr = ns == 0 ? c.swvdr : c.swidr, swdf = ns == 0 ? c.swvdf : c.swidf;
    double rupdir = ns == 0 ? cp01 : K::c0, rupdif = rupdir;
    double F[klevp + 1];
#pragma unroll
    for (int k = klevp; k >= 0; --k) {
      if (k < klevp) {
        const Layer& m = L[k];
        const double refkp1 = K::c1 / (K::c1 - m.rdif_b * rupdif);
        rupdir = m.rdir + (m.trnlay * rupdir + (m.tdir - m.trnlay) * rupdif) * refkp1 * m.tdif_b;
        rupdif = m.rdif_a + m.tdif_a * rupdif * refkp1 * m.tdif_b;
      }
      const double refk = K::c1 / (K::c1 - rdndif[k] * rupdif);
      const double fdirup = (trndir[k] * rupdir + (trntdr[k] - trndir[k]) * rupdif) * refk;
      const double fdirdn = trndir[k] + (trntdr[k] - trndir[k] + trndir[k] * rupdir * rdndif[k]) * refk;
      const double fdifup = trndif[k] * rupdif * refk;
      const double fdifdn = trndif[k] * refk;
      F[k] = (fdirdn - fdirup) * swdr + (fdifdn - fdifup) * swdf;
    }
    // (rupdir, rupdif are those of interface 0 now)
    // all absorbed flux above interface ksrf is surface absorption: 1 under snow, nslyr + 2 on bare or ponded ice
    const double Fsrf = srftyp == 1 ? F[1] : F[NSLYR + 2];
    if (ns == 0) {                           // visible (:2675-2746)
      o.avdr = rupdir;
      o.avdf = rupdif;
      o.fsfc = o.fsfc + F[0] - Fsrf;
      o.fint = o.fint + Fsrf - F[klevp];
      // (fthru + dir + dif, left to right: the two halves of F[klevp] are added to fthru = 0 one after the other)
      o.fthru = o.fthru + F[klevp];
      if (srftyp == 1) {
#pragma unroll
        for (int k = 1; k <= NSLYR; ++k) o.Sabs[k - 1] = o.Sabs[k - 1] + F[k] - F[k + 1];
      }
#pragma unroll
      for (int k = NSLYR + 2; k <= NSLYR + 1 + NILYR; ++k) {
        const double Fm = (srftyp == 1 && k == NSLYR + 2) ? F[k - 1] : F[k];
        o.Iabs[k - NSLYR - 2] = o.Iabs[k - NSLYR - 2] + Fm - F[k + 1];
      }
    } else {                                 // near infrared, two bands weighted (:2748-2832)
      const double w = ns == 1 ? wght2 : wght3;
      o.aidr = o.aidr + rupdir * w;
      o.aidf = o.aidf + rupdif * w;
      o.fsfc = o.fsfc + (F[0] - Fsrf) * w;
      o.fint = o.fint + (Fsrf - F[klevp]) * w;
      o.fthru = o.fthru + F[klevp] * w;
      if (srftyp == 1) {
#pragma unroll
        for (int k = 1; k <= NSLYR; ++k) o.Sabs[k - 1] = o.Sabs[k - 1] + (F[k] - F[k + 1]) * w;
      }
#pragma unroll
      for (int k = NSLYR + 2; k <= NSLYR + 1 + NILYR; ++k) {
        const double Fm = (srftyp == 1 && k == NSLYR + 2) ? F[k - 1] : F[k];
        o.Iabs[k - NSLYR - 2] = o.Iabs[k - NSLYR - 2] + (Fm - F[k + 1]) * w;
      }
    }
  }
}

// shortwave_dEdd_set_snow (:3554-3585) for a cell with aice > puny
CICE_HD inline void set_snow(double R_snw, double aice, double vsno, double Tsfc, double& fs, double* rhosnw, double* rsnw) {
  const double hs = vsno / aice;
  if (hs < hsmin)
    fs = K::c0;
  else if (hs <= hs0)
    fs = hs / hs0;
  else
    fs = K::c1;
  const double dTs = Timelt - Tsfc;
  const double fT = -dmin(dTs / dT_mlt - K::c1, K::c0);
  double rsnw_nm = rsnw_nonmelt - R_snw * rsnw_sig;
  rsnw_nm = dmax(rsnw_nm, rsnw_fresh);
  rsnw_nm = dmin(rsnw_nm, rsnw_melt);
#pragma unroll
  for (int k = 0; k < NSLYR; ++k) {
    rhosnw[k] = K::rhos;
    double r = rsnw_nm + (rsnw_melt - rsnw_nm) * fT;
    r = dmax(r, rsnw_fresh);
    rsnw[k] = dmin(r, rsnw_melt);
  }
}

// shortwave_dEdd_set_pond (:3668-3679)
CICE_HD inline void set_pond(double Tsfc, double fs, double& fp, double& hp) {
  const double dTs = Timelt - Tsfc;
  const double fT = -dmin(dTs / dT_mlt - K::c1, K::c0);
  fp = 0.3 * fT * (K::c1 - fs);
  hp = 0.3 * fT * (K::c1 - fs);
}

// shortwave_dEdd (:1537-1723) for one listed cell with aice > puny and coszen > puny.  hs, hi, fi, srftyp are this
// function's locals, carried from pass to pass as the reference's block arrays are: hs is 0 during the bare-ice pass and
// vsno / aice from the snow pass on; hi is reset to 0 in front of the pond pass and set again.
CICE_HD inline void dedd_column(const DeddParams& p, const Col& c, ColOut& o) {
  double fnidr = K::c0;
  if (c.swidr + c.swidf > K::puny) fnidr = c.swidr / (c.swidr + c.swidf);
  double hs = K::c0, hi = K::c0;
  hi = c.vice / c.aice;
  const double fi = K::c1 - c.fs - c.fp;
  Pass r;
#pragma unroll 1
  for (int srftyp = 0; srftyp < 3; ++srftyp) {
    double frac;
    bool take;
    if (srftyp == 0) {
      frac = fi;
      take = fi > K::c0;
    } else if (srftyp == 1) {
      hs = c.vsno / c.aice;
      frac = c.fs;
      take = c.fs > K::c0;
    } else {
      hi = K::c0;
      hi = c.vice / c.aice;
      frac = c.fp;
      take = c.fp > K::puny && c.hp > hpmin;
    }
    if (!take) continue;
    compute_pass(p, c, srftyp, hs, hi, fnidr, r);
    o.fswsfc = o.fswsfc + r.fsfc * frac;
    o.fswint = o.fswint + r.fint * frac;
    o.fswthru = o.fswthru + r.fthru * frac;
#pragma unroll
    for (int k = 0; k < NSLYR; ++k) o.Sswabs[k] = o.Sswabs[k] + r.Sabs[k] * frac;
#pragma unroll
    for (int k = 0; k < NILYR; ++k) o.Iswabs[k] = o.Iswabs[k] + r.Iabs[k] * frac;
    o.alvdr = o.alvdr + r.avdr * frac;
    o.alvdf = o.alvdf + r.avdf * frac;
    o.alidr = o.alidr + r.aidr * frac;
    o.alidf = o.alidf + r.aidf * frac;
    const double hist = K::c0 + p.awtvdr * r.avdr + p.awtidr * r.aidr + p.awtvdf * r.avdf + p.awtidf * r.aidf;
    if (srftyp == 0) o.albice = hist;
    else if (srftyp == 1) o.albsno = hist;
    else o.albpnd = hist;
  }
}

__device__ inline bool physical(const int32_t* blk, int b, int q, int nx) {
  const int i = q % nx + 1, j = q / nx + 1;
  const int32_t* w = blk + 4 * b;
  return i >= w[0] && i <= w[1] && j >= w[2] && j <= w[3];
}

// Grid (chunks of 256 cells of a plane, categories, blocks), as k_shortwave_ccsm3.  The register need allows one workgroup
// of four wavefronts per CU, a wavefront per SIMD.
__global__ __launch_bounds__(256) void k_shortwave_dedd(const DeddArgs a) {
  const int q = (int)(blockIdx.x * 256u + threadIdx.x);
  if (q >= a.np) return;
  const int n = (int)blockIdx.y, b = (int)blockIdx.z;
  const size_t np = (size_t)a.np;
  const size_t cb = (size_t)b * a.ncat + n;          // (category, block)
  const size_t c = cb * np + q, c2 = (size_t)b * np + q;
  const double aicen = a.aicen[c];
  const double coszen = a.coszen[c2];
  const bool on = (a.listed ? a.listed[q] != 0 : physical(a.blk, b, q, a.nx)) && aicen > K::puny;

  ColOut o;
  o.alvdr = o.alvdf = o.alidr = o.alidf = o.fswsfc = o.fswint = o.fswthru = o.albice = o.albsno = o.albpnd = K::c0;
#pragma unroll
  for (int k = 0; k < NSLYR; ++k) o.Sswabs[k] = K::c0;
#pragma unroll
  for (int k = 0; k < NILYR; ++k) o.Iswabs[k] = K::c0;

  if (on && coszen > K::puny) {
    Col col;
    col.aice = aicen; col.vice = a.vicen[c]; col.vsno = a.vsnon[c]; col.coszen = coszen;
    col.swvdr = a.swvdr[c2]; col.swvdf = a.swvdf[c2]; col.swidr = a.swidr[c2]; col.swidf = a.swidf[c2];
    if (a.snow_given) {
      col.fs = a.fs[c]; col.fp = a.fp[c]; col.hp = a.hp[c];
#pragma unroll
      for (int k = 0; k < NSLYR; ++k) {
        col.rhosnw[k] = a.rhosnw[(cb * NSLYR + k) * np + q];
        col.rsnw[k] = a.rsnw[(cb * NSLYR + k) * np + q];
      }
    } else {
      const double Tsfc = a.Tsfc[cb * a.tsfc_planes * np + q];
      set_snow(a.p.R_snw, aicen, col.vsno, Tsfc, col.fs, col.rhosnw, col.rsnw);
      if (a.p.tr_pond) {
        col.fp = a.fp[c]; col.hp = a.hp[c];
      } else {
        set_pond(Tsfc, col.fs, col.fp, col.hp);
      }
    }
    dedd_column(a.p, col, o);
  }

  a.alvdrn[c] = o.alvdr; a.alvdfn[c] = o.alvdf; a.alidrn[c] = o.alidr; a.alidfn[c] = o.alidf;
  a.fswsfcn[c] = o.fswsfc; a.fswintn[c] = o.fswint; a.fswthrun[c] = o.fswthru;
  a.albicen[c] = o.albice; a.albsnon[c] = o.albsno; a.albpndn[c] = o.albpnd;
#pragma unroll
  for (int k = 0; k < NSLYR; ++k) a.Sswabsn[(cb * NSLYR + k) * np + q] = o.Sswabs[k];
#pragma unroll
  for (int k = 0; k < NILYR; ++k) a.Iswabsn[(cb * NILYR + k) * np + q] = o.Iswabs[k];
}

// one surface or layer of the tuning: sigp with the scattering scaled, then k and w (:2359-2361 and its neighbours)
void tune_one(double k_mn, double w_mn, double factor, bool clamp, double& k, double& w) {
  double sigp = k_mn * w_mn * factor;
  if (clamp) sigp = sigp > K::c0 ? sigp : K::c0;   // max(sigp, c0): the branches for R < 0
  k = sigp + k_mn * (K::c1 - w_mn);
  w = sigp / k;
}

}  // namespace

void dedd_tune(DeddParams& p, double R_ice, double R_pnd) {
  const double fp_ice = 0.15, fm_ice = 0.15, fp_pnd = 2.00, fm_pnd = 0.50;
  const bool neg_i = !(R_ice >= K::c0), neg_p = !(R_pnd >= K::c0);
  const double f_i = neg_i ? K::c1 + fm_ice * R_ice : K::c1 + fp_ice * R_ice;
  const double f_p = neg_p ? K::c1 + fm_pnd * R_pnd : K::c1 + fp_pnd * R_pnd;
  for (int ns = 0; ns < nspint; ++ns) {
    tune_one(ki_ssl_mn[ns], wi_ssl_mn[ns], f_i, neg_i, p.ki_ssl[ns], p.wi_ssl[ns]);
    tune_one(ki_dl_mn[ns], wi_dl_mn[ns], f_i, neg_i, p.ki_dl[ns], p.wi_dl[ns]);
    tune_one(ki_int_mn[ns], wi_int_mn[ns], f_i, neg_i, p.ki_int[ns], p.wi_int[ns]);
    tune_one(ki_p_ssl_mn[ns], wi_p_ssl_mn[ns], f_p, neg_p, p.ki_p_ssl[ns], p.wi_p_ssl[ns]);
    tune_one(ki_p_int_mn[ns], wi_p_int_mn[ns], f_p, neg_p, p.ki_p_int[ns], p.wi_p_int[ns]);
    p.gi_ssl[ns] = gi_ssl_mn[ns]; p.gi_dl[ns] = gi_dl_mn[ns]; p.gi_int[ns] = gi_int_mn[ns];
    p.gi_p_ssl[ns] = gi_p_ssl_mn[ns]; p.gi_p_int[ns] = gi_p_int_mn[ns];
  }
}

void dedd_launch(const DeddArgs& a, hipStream_t s) {
  CICE_REQUIRE(a.nx >= 1 && a.np >= a.nx && a.np % a.nx == 0 && a.ncat >= 1 && a.nb >= 1, "shortwave_dEdd: bad dimensions");
  CICE_REQUIRE((long long)a.np < (1ll << 31) - 256 && a.ncat <= 65535 && a.nb <= 65535, "shortwave_dEdd: bad dimensions");
  CICE_REQUIRE(a.listed || a.blk, "shortwave_dEdd: no list");
  CICE_REQUIRE(!a.listed || (a.ncat == 1 && a.nb == 1), "shortwave_dEdd: a list names the cells of one block and category");
  CICE_REQUIRE(a.aicen && a.vicen && a.vsnon && a.coszen && a.swvdr && a.swvdf && a.swidr && a.swidf && a.alvdrn && a.alvdfn &&
                   a.alidrn && a.alidfn && a.fswsfcn && a.fswintn && a.fswthrun && a.Sswabsn && a.Iswabsn && a.albicen &&
                   a.albsnon && a.albpndn, "shortwave_dEdd: NULL buffer");
  if (a.snow_given)
    CICE_REQUIRE(a.fs && a.rhosnw && a.rsnw && a.fp && a.hp, "shortwave_dEdd: NULL buffer");
  else
    CICE_REQUIRE(a.tsfc_planes >= 1 && a.Tsfc && (!a.p.tr_pond || (a.fp && a.hp)), "shortwave_dEdd: NULL buffer");
  const dim3 grid((unsigned)((a.np + 255) / 256), (unsigned)a.ncat, (unsigned)a.nb);
  hipLaunchKernelGGL(k_shortwave_dedd, grid, dim3(256), 0, s, a);
  CICE_HIP(hipGetLastError());
}

}  // namespace cice
