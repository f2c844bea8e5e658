// CPU harness of ampligraph_amd/csrc/kge_loss.h (tests/test_loss_host.py): the product's Loss.__call__ template, compiled by g++ and
// run over the serial walk -- the walk of cols_loss_kernel, here with the scores of one positive 3 floats apart.
//   in : any number of problems  kind margin alpha reduction_mean eta P n_0 .. n_eta-1   (floats as strtof reads them: decimal,
//        hex, inf, nan)
//   out: per problem one line  per dP c_0 .. c_eta-1  as hex floats (-0.0 prints as -0x0p+0)
#include <stdio.h>

#include <vector>

#include "../../ampligraph_amd/csrc/kge_loss.h"

int main() {
    constexpr int64_t STRIDE = 3;
    int kind, mean, eta;
    float margin, alpha, P;
    while (scanf("%d %f %f %d %d %f", &kind, &margin, &alpha, &mean, &eta, &P) == 6) {
        if (eta < 1) return 2;
        std::vector<float> buf((size_t)eta * STRIDE + 1, -12345.f);
        for (int j = 0; j < eta; ++j)
            if (scanf("%f", &buf[1 + (size_t)j * STRIDE]) != 1) return 2;
        amdkge_loss L{};
        L.kind = kind; L.margin = margin; L.alpha = alpha; L.reduction_mean = mean;
        float per, dP;
        kge::loss_call(L, P, eta, kge::SerialWalk{buf.data() + 1, STRIDE, 1.f}, per, dP);
        printf("%a %a", per, dP);
        for (int j = 0; j < eta; ++j) printf(" %a", buf[1 + (size_t)j * STRIDE]);
        printf("\n");
        for (size_t q = 0; q < buf.size(); ++q)
            if ((q + 2) % STRIDE != 0 && buf[q] != -12345.f) return 3;   // the walk wrote between its scores
    }
    return 0;
}
