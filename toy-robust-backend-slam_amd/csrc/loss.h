#pragma once
// Ceres 2.x LossFunction::Evaluate for the loss family of pgo_set_losses (include/pgo.h, "robust losses"): ONE statement
// of the formulas, evaluated by K1 on the device (k_edge_eval's general instantiation) and by pgo_loss_evaluate on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pgo.h"

namespace pgo {

constexpr int MAX_LOSS_CLASSES = 4;   // an edge's class sits in bits 2-3 of its flags byte
constexpr double LOSS_DBL_MIN = 2.2250738585072014e-308;

// one loss class as K1 reads it: the type and the constants of its formulas
struct LossClass {
  int32_t type;
  int32_t _pad;
  double a, b, c;
};

// b and c as the Ceres constructors derive them (only the ones the type uses are meaningful)
inline LossClass make_loss_class(int32_t type, double a) {
  LossClass L;
  L.type = type;
  L._pad = 0;
  L.a = a;
  L.b = 0.0;
  L.c = 0.0;
  switch (type) {
    case PGO_LOSS_HUBER: L.b = a * a; break;
    case PGO_LOSS_SOFTLONE:
    case PGO_LOSS_CAUCHY: L.b = a * a; L.c = 1.0 / L.b; break;
    case PGO_LOSS_ARCTAN: L.b = 1.0 / (a * a); break;
    case PGO_LOSS_TUKEY: L.b = a * a; break;   // a^2
    default: L.a = 0.0; break;                 // Trivial ignores a
  }
  return L;
}

// rho[0..2] = rho(s), rho'(s), rho''(s)
__host__ __device__ inline void loss_rho(const LossClass& L, double s, double rho[3]) {
  const double a = L.a, b = L.b, c = L.c;
  switch (L.type) {
    case PGO_LOSS_HUBER:
      if (s > b) {
        const double r = sqrt(s);
        rho[0] = 2.0 * a * r - b;
        rho[1] = fmax(LOSS_DBL_MIN, a / r);
        rho[2] = -rho[1] / (2.0 * s);
      } else {
        rho[0] = s;
        rho[1] = 1.0;
        rho[2] = 0.0;
      }
      return;
    case PGO_LOSS_SOFTLONE: {
      const double sum = 1.0 + s * c, tmp = sqrt(sum);
      rho[0] = 2.0 * b * (tmp - 1.0);
      rho[1] = fmax(LOSS_DBL_MIN, 1.0 / tmp);
      rho[2] = -(c * rho[1]) / (2.0 * sum);
      return;
    }
    case PGO_LOSS_CAUCHY: {
      const double sum = 1.0 + s * c, inv = 1.0 / sum;
      rho[0] = b * log(sum);
      rho[1] = fmax(LOSS_DBL_MIN, inv);
      rho[2] = -c * (inv * inv);
      return;
    }
    case PGO_LOSS_ARCTAN: {
      const double sum = 1.0 + s * s * b, inv = 1.0 / sum;
      rho[0] = a * atan2(s, a);
      rho[1] = fmax(LOSS_DBL_MIN, inv);
      rho[2] = -2.0 * s * b * (inv * inv);
      return;
    }
    case PGO_LOSS_TUKEY:
      if (s <= b) {
        const double v = 1.0 - s / b, v2 = v * v;
        rho[0] = b / 3.0 * (1.0 - v2 * v);
        rho[1] = v2;
        rho[2] = -2.0 / b * v;
      } else {
        rho[0] = b / 3.0;
        rho[1] = 0.0;
        rho[2] = 0.0;
      }
      return;
    default:   // PGO_LOSS_TRIVIAL
      rho[0] = s;
      rho[1] = 1.0;
      rho[2] = 0.0;
      return;
  }
}

// a valid pgo_loss: a known type, and a finite scale > 0 unless Trivial
inline bool loss_valid(const pgo_loss& l) {
  if (l.type < PGO_LOSS_TRIVIAL || l.type > PGO_LOSS_TUKEY) return false;
  return l.type == PGO_LOSS_TRIVIAL || (std::isfinite(l.a) && l.a > 0.0);
}

}  // namespace pgo
