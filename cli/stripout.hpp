// --strip for the CLIs that know key frames: every exported key frame goes into a uw::Strip where the program writes it
// (main.cpp:294,377), and at the end of the input each segment is rendered and written as <prefix>strip_NNN.<ext>, with one
// line per segment after the report's table:  Strip:\t<file>\t<first ID>\t<count>\t<cols> x <rows>
#pragma once
#include <memory>
#include <ostream>
#include "cliutil.hpp"

struct StripOut {
    bool on = false;
    int mode = UWIP_STRIP_FEATHER;
    int max_frames = 1024;
    bool gain = false;                            // --strip-gain: gain compensation from the overlaps of consecutive key frames
    int levels = 4;                               // --strip-levels: levels of the stacks of --strip-mode multiband (ramps 1, 2, 4, 8)
    int seam_prior = 1024;                        // --strip-seam-prior: uwip_strip_seam_config.prior of --strip-mode seam
    unsigned detect_flags = 0, match_flags = 0;
    std::shared_ptr<uw::Strip> strip;             // made at the first key frame; declare a StripOut after its context

    // --strip [--strip-mode feather|first|last|multiband|seam] [--strip-levels N] [--strip-seam-prior N] [--strip-max N]
    // [--strip-gain]; false: an unknown mode, levels outside 1..4 or a prior outside 0..4096.  --strip-gain without --strip is the caller's to refuse (gain_without_strip)
    bool configure(const Args &a)
    {
        on = a.has("strip");
        gain = a.has("strip-gain");
        const std::string m = a.get("strip-mode", "feather");
        if (m == "feather") mode = UWIP_STRIP_FEATHER;
        else if (m == "first") mode = UWIP_STRIP_FIRST;
        else if (m == "last") mode = UWIP_STRIP_LAST;
        else if (m == "multiband") mode = UWIP_STRIP_MULTIBAND;
        else if (m == "seam") mode = UWIP_STRIP_SEAM;
        else return false;
        levels = std::atoi(a.get("strip-levels", "4").c_str());
        if (levels < 1 || levels > 4) return false;
        const std::string p = a.get("strip-seam-prior", "1024");
        if (p.empty() || p.find_first_not_of("0123456789") != std::string::npos || p.size() > 4) return false;
        seam_prior = std::atoi(p.c_str());
        if (seam_prior > 4096) return false;
        max_frames = std::max(1, std::atoi(a.get("strip-max", "1024").c_str()));
        return true;
    }
    bool gain_without_strip() const { return gain && !on; }
    void add(uw::Context &ctx, imgio::Image &im)
    {
        if (!on) return;
        if (!strip) strip.reset(new uw::Strip(ctx, im.rows, im.cols, max_frames, detect_flags, match_flags));
        strip->add(as_mat(im));
    }
    void finish(const std::string &prefix, const char *ext, std::ostream &report)
    {
        if (!on || !strip) return;
        const std::vector<uwip_strip_segment> segs = strip->layout();
        if (gain) strip->gains();
        if (mode == UWIP_STRIP_MULTIBAND) {               // after the last add: the stacks of every key frame
            uwip_strip_bands_config bc;
            uwip_strip_bands_config_default(&bc);
            bc.levels = levels;
            strip->bands(&bc);
        }
        if (mode == UWIP_STRIP_SEAM) {                    // after the gains: the costs are those of the gained frames
            uwip_strip_seam_config sc;
            uwip_strip_seam_config_default(&sc);
            sc.prior = seam_prior;
            strip->seams(&sc);
        }
        for (size_t i = 0; i < segs.size(); ++i) {
            uw::Mat m;
            imgio::Image im;
            strip->render((int)i, gain ? mode | UWIP_STRIP_GAIN : mode, m, im.data);
            im.rows = m.rows; im.cols = m.cols; im.channels = 3;
            char name[512];
            std::snprintf(name, sizeof name, "%sstrip_%03zu.%s", prefix.c_str(), i, ext);
            if (!imgio::imwrite(name, im)) throw uw::Error(UWIP_ERR_INVALID, std::string("cannot write ") + name);
            std::printf("Strip: %s  key frames %d..%d  %d x %d\n", name, segs[i].first, segs[i].first + segs[i].count - 1, segs[i].cols, segs[i].rows);
            report << "Strip:\t" << name << "\t" << segs[i].first << "\t" << segs[i].count << "\t" << segs[i].cols << " x " << segs[i].rows << "\n";
        }
    }
};
