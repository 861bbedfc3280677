// sweep_plan_driver.cpp -- the host-side sweep planner (genome-downsampler_amd/csrc/sweep_plan.h) on the CPU, for
// tests/test_sweep_plan_cpu.py.  One shape per line of stdin, a route and key=value fields; one line of key=value fields
// of the plan per shape on stdout:
//   uniform n= span= ltot= contigs= M= empty=                        plan_uniform_sweep (empty: 4294967295 = unknown)
//   near    n= ell= min_span= ltot= contigs= longest= M= may_rank=   plan_near_uniform
//   mixed   n= span= ltot= contigs= M= in_regs= hopeless=            plan_mixed_sweep, and where the plan samples the
//           [s0= s1= s2= longest=]                                   spans and s0 is given, refine_mixed_with_span_sample
//   share   reads= positions= contigs= span= M=                      share_sweeps_as_stretches
//   sizes   contigs= windows= tier= ltot= ell= wg= cand=             the stretch tables' words and a tier's offset, the
//                                                                    event-driven form's scratch, the boundary snapshots
// Options on any line: sweep= cuts= spec= run_in= nu_min_depth= (qmcp_hip_options: sweep, cut_points, speculation,
// speculation_run_in, near_uniform_min_depth).
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "sweep_plan.h"

static const char* form_name(qmcp::UniformForm f) {
    switch (f) {
        case qmcp::UniformForm::Events: return "events";
        case qmcp::UniformForm::SpeculativeGeneral: return "spec_general";
        case qmcp::UniformForm::General: return "general";
        case qmcp::UniformForm::Fast: return "fast";
        case qmcp::UniformForm::SingleWave: return "single_wave";
    }
    return "?";
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string route, tok;
        if (!(in >> route)) continue;
        std::map<std::string, double> f;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq != std::string::npos) f[tok.substr(0, eq)] = std::stod(tok.substr(eq + 1));
        }
        auto get = [&](const char* k, double dflt = 0.0) { return f.count(k) ? f[k] : dflt; };
        auto u32 = [&](const char* k, double dflt = 0.0) { return (uint32_t)get(k, dflt); };
        qmcp_hip_options opt = {};
        opt.struct_size = sizeof(opt);
        opt.sweep = (int32_t)get("sweep");
        opt.cut_points = (int32_t)get("cuts");
        opt.speculation = (int32_t)get("spec");
        opt.speculation_run_in = u32("run_in");
        opt.near_uniform_min_depth = (float)get("nu_min_depth");
        if (route == "uniform") {
            const qmcp::UniformSweepPlan p = qmcp::plan_uniform_sweep(opt, u32("n"), u32("span"), u32("ltot"), u32("contigs"),
                                                                      u32("M"), u32("empty", 4294967295.0));
            std::printf("form=%s windows=%u speculate=%d burn_blocks=%u unit=%u round_to=%u run_ins_apart=%u min_run_ins=%u\n",
                        form_name(p.form), p.windows, (int)p.speculate, p.burn_blocks, p.unit, p.round_to,
                        qmcp::UniformSweepPlan::run_ins_apart, qmcp::UniformSweepPlan::min_run_ins);
        } else if (route == "near") {
            const qmcp::NearUniformPlan p = qmcp::plan_near_uniform(opt, u32("n"), u32("ell"), u32("min_span"), u32("ltot"),
                                                                    u32("contigs"), u32("longest"), u32("M"),
                                                                    get("may_rank", 1.0) != 0.0);
            std::printf("tried=%d stretches=%d speculate=%d burn_blocks=%u windows=%u\n", (int)p.tried, (int)p.stretches,
                        (int)p.speculate, p.burn_blocks, p.windows);
        } else if (route == "mixed") {
            qmcp::MixedSweepPlan p = qmcp::plan_mixed_sweep(opt, u32("n"), u32("span"), u32("ltot"), u32("contigs"), u32("M"),
                                                            get("in_regs", 1.0) != 0.0, get("hopeless") != 0.0);
            const bool sample = p.sample_span_mode;
            if (sample && f.count("s0")) {
                const uint32_t share[3] = {u32("s0"), u32("s1"), u32("s2")};
                p = qmcp::refine_mixed_with_span_sample(opt, p, share, u32("longest"));
            }
            std::printf("windows=%u sample=%d speculate=%d burn_blocks=%u round_to=%u run_ins_apart=%u min_run_ins=%u\n",
                        p.windows, (int)sample, (int)p.speculate, p.burn_blocks, qmcp::MixedSweepPlan::round_to,
                        qmcp::MixedSweepPlan::run_ins_apart, qmcp::MixedSweepPlan::min_run_ins);
        } else if (route == "share") {
            std::printf("stretches=%d\n", (int)qmcp::share_sweeps_as_stretches(get("reads"), get("positions"),
                                                                              (size_t)get("contigs"), u32("span"), u32("M")));
        } else if (route == "sizes") {
            const uint32_t contigs = u32("contigs"), windows = u32("windows"), ltot = u32("ltot"), ell = u32("ell", 1.0),
                           wg = u32("wg");
            std::printf("words=%zu offset=%zu pieces=%u pack_bytes=%zu ckpt_bytes=%zu last_bytes=%zu ev_wg_max=%u "
                        "snap_bytes=%zu\n",
                        qmcp::sweep_segment_words(contigs, windows),
                        qmcp::sweep_segment_table_offset(contigs, windows, u32("tier")), qmcp::sweep_ev_pieces(ltot, ell, wg),
                        qmcp::sweep_ev_pack_bytes(ltot, ell, wg), qmcp::sweep_ev_ckpt_bytes(ltot, ell, wg),
                        qmcp::sweep_ev_last_bytes(ltot, ell, wg), qmcp::sweep_ev_workgroups_max(contigs),
                        qmcp::spec_snap_bytes(u32("cand")));
        } else {
            std::printf("error=unknown_route\n");
        }
    }
    return 0;
}
