// Reader of the text descriptor of the stand-alone host programs (layout_probe.cpp,
// gram_tables_check.cpp): one linear GPC scenario as whitespace-separated numbers on stdin,
//   my nu nit n2_max nu_max
//   n1[my]
//   my*nu plant entries, row-major, each `len num[len] den[len] delay`
//   my*nu model entries, the same way
//   du_min[nu] du_max[nu] u_min[nu] u_max[nu]
// filled into an mpct_scenario_desc without CARIMA tables (the library derives them from the model).
// A band scenario (mdband_kernel.hip; written by tests/band_family.py descriptor_text) starts with
// the word `band` and its number of measured disturbances, has my*(nu+nd) entries per table and ends
// with the output bands:
//   band nd
//   my nu nit n2_max nu_max ... u_max[nu]           (as above)
//   y_min[my] y_max[my] ecr_min[my] ecr_max[my] rho
#pragma once
#include "scenario_tables.h"

#include <cstdio>
#include <iostream>
#include <string>

struct TextDescriptor {
  struct Entries {
    std::vector<std::vector<double>> num, den;
    std::vector<mpct_dtf> tf;
    bool read(int n) {
      num.resize(n);
      den.resize(n);
      tf.resize(n);
      for (int e = 0; e < n; ++e) {
        int len = 0, delay = 0;
        if (!(std::cin >> len) || len < 1 || len > 64) return false;
        num[e].resize(len);
        den[e].resize(len);
        for (double& x : num[e])
          if (!(std::cin >> x)) return false;
        for (double& x : den[e])
          if (!(std::cin >> x)) return false;
        if (!(std::cin >> delay)) return false;
        tf[e] = {len, num[e].data(), den[e].data(), delay};
      }
      return true;
    }
  };
  static bool read_vec(std::vector<double>& v, int n) {
    v.resize(n);
    for (double& x : v)
      if (!(std::cin >> x)) return false;
    return true;
  }

  int my = 0, nu = 0, nit = 0, n2max = 0, numax = 0, nd = 0;
  bool band = false;
  std::vector<int32_t> n1;
  Entries plant, model;
  std::vector<double> dumin, dumax, umin, umax, yref, ymin, ymax, ecrmin, ecrmax;
  double rho = 0.0;
  mpct_scenario_desc d{};

  // false (with a message printed) on a malformed descriptor
  bool read() {
    std::cin >> std::ws;
    if (std::cin.peek() == 'b') {
      std::string word;
      if (!(std::cin >> word >> nd) || word != "band" || nd < 0) {
        std::printf("malformed descriptor: band header\n");
        return false;
      }
      band = true;
    }
    if (!(std::cin >> my >> nu >> nit >> n2max >> numax) || my < 1 || my > mpct::kMaxOut || nu < 1 ||
        nu + nd > mpct::kMaxIn || nit < 1) {
      std::printf("malformed descriptor: dims\n");
      return false;
    }
    n1.resize(my);
    for (int32_t& x : n1)
      if (!(std::cin >> x)) {
        std::printf("malformed descriptor: n1\n");
        return false;
      }
    if (!plant.read(my * (nu + nd)) || !model.read(my * (nu + nd)) || !read_vec(dumin, nu) || !read_vec(dumax, nu) ||
        !read_vec(umin, nu) || !read_vec(umax, nu)) {
      std::printf("malformed descriptor: entries / bounds\n");
      return false;
    }
    yref.assign((size_t)my * nit, 0.0);
    d.abi_version = MPCT_ABI_VERSION;
    d.my = my;
    d.nu = nu;
    d.nit = nit;
    d.n2_max = n2max;
    d.nu_max = numax;
    d.weights_squared = 1;
    d.vns_ink = 10;
    d.n1 = n1.data();
    d.plant = plant.tf.data();
    d.model = model.tf.data();
    d.du_min = dumin.data();
    d.du_max = dumax.data();
    d.u_min = umin.data();
    d.u_max = umax.data();
    d.yref = yref.data();
    if (band) {
      if (!read_vec(ymin, my) || !read_vec(ymax, my) || !read_vec(ecrmin, my) || !read_vec(ecrmax, my) ||
          !(std::cin >> rho)) {
        std::printf("malformed descriptor: bands\n");
        return false;
      }
      d.nd = nd;
      d.mdband = 1;
      d.y_min = ymin.data();
      d.y_max = ymax.data();
      d.ecr_min = ecrmin.data();
      d.ecr_max = ecrmax.data();
      d.rho_ecr = rho;
    }
    return true;
  }
};
