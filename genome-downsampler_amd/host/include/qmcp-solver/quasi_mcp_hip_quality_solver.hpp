// "quasi-mcp-hip-quality": quasi-mcp-hip's coverage and number of reads, with the best reads.
// The reference's qmcp-cpu weighs reads by quality (libs/qmcp-solver/src/qmcp_cpu_cost_scaling_solver.cpp); this solver
// keeps, within every set of reads sharing (contig, start, end), as many reads as quasi-mcp-hip keeps there, chosen by
// quality descending, then read index (qmcp_hip_solve_quality_* in include/qmcp_hip.h).  uses_quality_of_reads() is
// true, so the app grades amplicon pairs instead of filtering them (src/app.cpp:120-128).
// Not registered by SolverManager's constructor: an embedding application adds it,
//     manager.add("quasi-mcp-hip-quality", std::make_unique<qmcp::QuasiMcpHipQualitySolver>());
#ifndef QMCP_AMD_QUASI_MCP_HIP_QUALITY_SOLVER_HPP
#define QMCP_AMD_QUASI_MCP_HIP_QUALITY_SOLVER_HPP

#include "qmcp-solver/quasi_mcp_hip_solver.hpp"

namespace qmcp {

class QuasiMcpHipQualitySolver : public QuasiMcpHipSolver {
   public:
    QuasiMcpHipQualitySolver() = default;  // trivial, like its base: the device is touched on the first solve

    std::unique_ptr<Solution> solve(std::uint32_t required_cover, bam_api::BamApi& bam_api) override;
    bool uses_quality_of_reads() override { return true; }

    const qmcp_hip_quality_stats& last_quality_stats() const { return qstats_; }

   protected:
    const char* name() const override { return "quasi-mcp-hip-quality"; }

   private:
    qmcp_hip_quality_stats qstats_{};
};

}  // namespace qmcp
#endif
