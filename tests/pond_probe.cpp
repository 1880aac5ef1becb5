// Stand-alone host program around pond_cell (cice4_amd/csrc/pond_cell.h) for tests/test_pond_golden.py.
// usage: pond_probe IN OUT.  IN: doubles -- n, ponds, age, dt, then n records of the nine words of PondIn (aicen, vicen,
// vsnon, Tsfc, meltt, melts, frain, volpn, iage).  OUT: n records of five doubles -- apondn, hpondn, volpn, iage and the
// POND_ST_* mask of the words pond_cell asks its caller to store.
#include <cstdio>
#include <vector>

#include "../cice4_amd/csrc/pond_cell.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  double head[4];
  if (std::fread(head, 8, 4, f) != 4) return 4;
  const size_t n = (size_t)head[0];
  const bool ponds = head[1] != 0.0, age = head[2] != 0.0;
  const double dt = head[3];
  std::vector<double> in(9 * n), out(5 * n);
  if (std::fread(in.data(), 8, in.size(), f) != in.size()) return 4;
  std::fclose(f);
  for (size_t k = 0; k < n; ++k) {
    const double* w = &in[9 * k];
    const cice::PondIn p{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]};
    const cice::PondOut o = cice::pond_cell(ponds, age, dt, p);
    double* r = &out[5 * k];
    r[0] = o.apondn; r[1] = o.hpondn; r[2] = o.volpn; r[3] = o.iage; r[4] = (double)o.st;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  if (std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 6;
  std::fclose(f);
  std::printf("cells=%zu\n", n);
  return 0;
}
