#!/usr/bin/env python3
"""tools/diff_fuzz_scenes.py — differential fuzzing of the restated path against the reference itself.

    python tools/diff_fuzz_scenes.py [--n 200] [--seed 0] [--keep DIR]

Writes random small scenes (random camera, sampler, filter, film / sensor parameters, lights, textures, materials, shapes, object
instances, media — combinations no hand-written golden has), renders each with oracle/_ref/pbrt_ref --wavefront (the unmodified
reference built here) and with oracle/_build/wf_cpu (the stage bodies the HIP kernels run, compiled for the host) and compares the
images BIT FOR BIT, or the fact that both refuse the scene.  A difference is a parity bug in code the GPU shares: the scene is kept.
Needs /root/reference's build (oracle/_ref); test infrastructure only."""
import argparse
import os
import random
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import read_pfm  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "pbrt_ref")
CPU = os.path.join(ROOT, "oracle", "_build", "wf_cpu")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def f(*v):
    return " ".join("%.6g" % x for x in v)


class StressRandom(random.Random):
    """--stress: every `r.random() < p` of the grammar comes true with probability sqrt(p) — the rare features (rendering spaces, camera motion,
    media, animated shapes, emitters, odd film options) two to three times as often, and so their COMBINATIONS, which is where the findings
    of seeds 17 / 18 were (portal light x camera space, animated shape x interface surface x medium).  Values drawn with uniform() are not biased."""
    def random(self):
        return super().random() ** 2

    def uniform(self, a, b):
        return a + (b - a) * super().random()


STRESS = False
EXTENDED_OPTIONS = False
NESTED_ANIMATED = False   # --nested-animated: a definition may hold a moving entity (off: every seed generates the scene it always did)


class Gen:
    def __init__(self, seed):
        self.r = StressRandom(seed) if STRESS else random.Random(seed)
        self.float_tex, self.spec_tex, self.materials = [], [], []
        self.media = []

    def u(self, a=0.0, b=1.0):
        return self.r.uniform(a, b)

    def rgb(self, lo=0.05, hi=0.95):
        return "[ %s ]" % f(self.u(lo, hi), self.u(lo, hi), self.u(lo, hi))

    def pick(self, xs):
        return self.r.choice(xs)

    # ---- header -------------------------------------------------------------------------------------------------
    def header(self):
        r = self.r
        out = []
        if r.random() < 0.15:
            out.append('Option "rendercoordsys" "%s"' % self.pick(["camera", "cameraworld", "world"]))
        if EXTENDED_OPTIONS:
            # (round 5, last session; drawn only under --options so that the scenes of the earlier seeds can be regenerated) the other Option
            # directives of the path (scene.cpp BasicSceneBuilder::Option): bare-token values
            for name in ("disablepixeljitter", "disablewavelengthjitter", "disabletexturefiltering"):
                if r.random() < 0.08:
                    out.append('Option "%s" true' % name)
            if r.random() < 0.08:
                out.append('Option "seed" %d' % r.randrange(1, 1000))
            if r.random() < 0.08:
                out.append('Option "displacementedgescale" %s' % f(self.u(0.5, 2)))
        if r.random() < 0.1:
            out.append('ColorSpace "%s"' % self.pick(["srgb", "rec2020", "dci-p3", "aces2065-1"]))
        self.camera_motion = r.random() < 0.12   # (round 4, end) ActiveTransform StartTime / EndTime around the camera: AnimatedTransform
        # (round 5, end) the interval the animated transformations are defined over: inside, around and beside the shutter (times outside
        # it clamp to the start / end transformation; a subsurface exit continues at time 0, which -0.5 .. 1 puts in between)
        tt = self.pick(["0 1"] * 3 + ["-0.5 1", "0.2 0.7", "0 1.5", "-1 0.4"])
        if self.camera_motion or r.random() < 0.3:
            out.append("TransformTimes " + tt)
        if self.camera_motion:
            out.append("ActiveTransform StartTime")
        out.append("LookAt %s  %s  0 0 1" % (f(self.u(-1, 1), -7 + self.u(-1, 1), 2.5 + self.u(-1, 1)), f(self.u(-.5, .5), self.u(-.5, .5), 1 + self.u(-.3, .3))))
        if self.camera_motion:
            out.append("ActiveTransform EndTime")
            out.append("LookAt %s  %s  %s" % (f(self.u(-1, 1), -7 + self.u(-1, 1), 2.5 + self.u(-1, 1)), f(self.u(-.5, .5), self.u(-.5, .5), 1 + self.u(-.3, .3)), f(self.u(-0.1, 0.1), 0, 1)))
            out.append("ActiveTransform All")
        cam = self.pick(["perspective"] * 4 + ["orthographic", "spherical", "realistic"])
        if cam == "perspective":
            out.append('Camera "perspective" "float fov" [ %s ]' % f(self.u(25, 70)) +
                       (' "float lensradius" [ %s ] "float focaldistance" [ %s ]' % (f(self.u(0.01, 0.2)), f(self.u(4, 9))) if r.random() < 0.3 else "") +
                       (' "float shutteropen" [ 0.1 ] "float shutterclose" [ 0.8 ]' if r.random() < 0.2 else ""))
        elif cam == "orthographic":
            out.append('Camera "orthographic" "float screenwindow" [ -4 4 -3 3 ]' + (' "float lensradius" [ 0.05 ] "float focaldistance" [ 7 ]' if r.random() < 0.3 else ""))
        elif cam == "spherical":
            out.append('Camera "spherical" "string mapping" "%s"' % self.pick(["equalarea", "equirectangular"]))
        else:
            out.append('Camera "realistic" "string lensfile" "%s" "float aperturediameter" [ %s ] "float focusdistance" [ %s ]'
                       % (os.path.join(GOLDEN, "dgauss50.dat"), f(self.u(4, 17)), f(self.u(5, 9))))
        spp = self.pick([1, 2, 3, 4, 8])
        samp = self.pick(["zsobol"] * 3 + ["halton", "sobol", "paddedsobol", "independent", "stratified"])
        if samp == "stratified":
            out.append('Sampler "stratified" "integer xsamples" [ %d ] "integer ysamples" [ %d ] "bool jitter" %s' % (self.pick([1, 2, 3]), self.pick([1, 2]), self.pick(["true", "false"])))
        else:
            rnd = ""
            if samp in ("zsobol", "sobol", "paddedsobol") and r.random() < 0.5:
                rnd = ' "string randomization" "%s"' % self.pick(["none", "permutedigits", "fastowen", "owen"])
            if samp == "halton" and r.random() < 0.5:
                rnd = ' "string randomization" "%s"' % self.pick(["none", "permutedigits", "owen"])
            out.append('Sampler "%s" "integer pixelsamples" [ %d ]%s' % (samp, spp, rnd))
        out.append('Integrator "volpath" "integer maxdepth" [ %d ]' % self.pick([0, 1, 3, 5, 9]) + (' "bool regularize" true' if r.random() < 0.15 else "") +
                   (' "string lightsampler" "%s"' % self.pick(["bvh", "power", "uniform"]) if r.random() < 0.4 else ""))
        filt = self.pick(["gaussian", "box", "mitchell", "sinc", "triangle", None])
        if filt:
            out.append('PixelFilter "%s"' % filt + (' "float xradius" [ %s ] "float yradius" [ %s ]' % (f(self.u(0.5, 2.5)), f(self.u(0.5, 2.5))) if r.random() < 0.5 else ""))
        film = 'Film "rgb" "string filename" [ "fz.pfm" ] "integer xresolution" [ %d ] "integer yresolution" [ %d ] "bool savefp16" [ false ]' % (self.pick([16, 24, 33]), self.pick([12, 16, 19]))
        if r.random() < 0.2:
            film += ' "float iso" [ %s ]' % f(self.u(50, 400))
        if r.random() < 0.15:
            film += ' "float whitebalance" [ %s ]' % f(self.u(3000, 9000))
        if r.random() < 0.15:
            film += ' "string sensor" "%s"' % self.pick(["cie1931", "canon_eos_5d_mkiv", "nikon_d850", "sony_ilce_7rm3"])
        if r.random() < 0.15:
            film += ' "float maxcomponentvalue" [ %s ]' % f(self.u(0.5, 5))
        if r.random() < 0.15:
            film += ' "float cropwindow" [ 0.1 0.8 0.2 0.9 ]'
        out.append(film)
        if r.random() < 0.2:
            out.append('MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" %s "rgb sigma_s" %s "float scale" [ %s ] "float g" [ %s ]'
                       % (self.rgb(0.01, 0.2), self.rgb(0.01, 0.3), f(self.u(0.05, 0.5)), f(self.u(-0.6, 0.8))))
            self.media.append("fog")
        return out

    # ---- world --------------------------------------------------------------------------------------------------
    def spectrum_param(self, name, lo=0.05, hi=0.95):
        k = self.r.random()
        if k < 0.6 or not self.spec_tex:
            if k < 0.1:
                return '"spectrum %s" [ 300 %s 500 %s 800 %s ]' % (name, f(self.u(lo, hi)), f(self.u(lo, hi)), f(self.u(lo, hi)))
            return '"rgb %s" %s' % (name, self.rgb(lo, hi))
        return '"texture %s" "%s"' % (name, self.pick(self.spec_tex))

    def float_param(self, name, lo, hi):
        if self.float_tex and self.r.random() < 0.25:
            return '"texture %s" "%s"' % (name, self.pick(self.float_tex))
        return '"float %s" [ %s ]' % (name, f(self.u(lo, hi)))

    def mapping(self):
        m = self.pick(["uv", "uv", "spherical", "cylindrical", "planar"])
        s = ' "string mapping" "%s"' % m
        if m == "uv":
            s += ' "float uscale" [ %s ] "float vscale" [ %s ] "float udelta" [ %s ]' % (f(self.u(0.5, 6)), f(self.u(0.5, 6)), f(self.u(0, 1)))
        elif m == "planar":
            s += ' "vector3 v1" [ 1 0 0.2 ] "vector3 v2" [ 0 1 0.3 ]'
        return s

    def textures(self):
        out = []
        for i in range(self.r.randrange(0, 5)):
            name = "ft%d" % i
            kind = self.pick(["constant", "scale", "mix", "checkerboard", "fbm", "wrinkled", "windy", "dots", "bilerp", "imagemap", "directionmix"])
            if kind == "constant":
                out.append('Texture "%s" "float" "constant" "float value" [ %s ]' % (name, f(self.u(0, 1))))
            elif kind in ("scale", "mix", "directionmix") and self.float_tex:
                if kind == "scale":
                    if self.r.random() < 0.3:   # the other argument order (FloatScaledTexture::Create tries both)
                        out.append('Texture "%s" "float" "scale" "float tex" [ %s ] "texture scale" "%s"' % (name, f(self.pick([1.0, self.u(0.2, 1.5)])), self.pick(self.float_tex)))
                    else:
                        out.append('Texture "%s" "float" "scale" "texture tex" "%s" "float scale" [ %s ]' % (name, self.pick(self.float_tex), f(self.pick([1.0, self.u(0.2, 1.5)]))))
                elif kind == "mix":
                    out.append('Texture "%s" "float" "mix" "texture tex1" "%s" "float tex2" [ %s ] "float amount" [ %s ]' % (name, self.pick(self.float_tex), f(self.u()), f(self.u())))
                else:
                    out.append('Texture "%s" "float" "directionmix" "texture tex1" "%s" "float tex2" [ %s ] "vector3 dir" [ 0.3 0.2 1 ]' % (name, self.pick(self.float_tex), f(self.u())))
            elif kind == "checkerboard":
                out.append('Texture "%s" "float" "checkerboard" "float tex1" [ %s ] "float tex2" [ %s ]' % (name, f(self.u()), f(self.u())) + (' "integer dimension" 3' if self.r.random() < 0.3 else self.mapping()))
            elif kind in ("fbm", "wrinkled"):
                out.append('Texture "%s" "float" "%s" "integer octaves" [ %d ] "float roughness" [ %s ]' % (name, kind, self.pick([2, 5, 8]), f(self.u(0.3, 0.7))))
            elif kind == "windy":
                out.append('Texture "%s" "float" "windy"' % name)
            elif kind == "dots":
                out.append('Texture "%s" "float" "dots" "float inside" [ %s ] "float outside" [ %s ]' % (name, f(self.u()), f(self.u())) + self.mapping())
            elif kind == "bilerp":
                out.append('Texture "%s" "float" "bilerp" "float v00" [ %s ] "float v01" [ %s ] "float v10" [ %s ] "float v11" [ %s ]' % (name, f(self.u()), f(self.u()), f(self.u()), f(self.u())))
            elif kind == "imagemap":
                # ("octahedralsphere" is no longer drawn: the ground quad's (u, v) run to 4 and a bump lookup steps beyond 1 — outside [0, 1]^2 by
                #  more than a texel the reference reads past its pixel array (below); s800146 was that, not a parity finding.  The wrap mode
                #  has its goldens.)
                wrap = self.pick(["repeat", "clamp", "black"])
                # (an octahedral map addressed outside [0, 1]^2 by more than a texel makes the reference read past its pixel array,
                #  util/image.h:100-121: undefined there — only the plain (u, v) mapping with it)
                out.append('Texture "%s" "float" "imagemap" "string filename" "%s" "string filter" "%s" "string wrap" "%s"'
                           % (name, os.path.join(GOLDEN, self.pick(["alpha.pfm", "bump.pfm", "png_grey8.png"])), self.pick(["bilinear", "point", "trilinear", "ewa"]), wrap) +
                           (' "string mapping" "uv"' if wrap == "octahedralsphere" else self.mapping()) +
                           (' "float scale" [ %s ]' % f(self.u(0.3, 1.4)) if self.r.random() < 0.3 else "") + (' "bool invert" true' if self.r.random() < 0.2 else "") +
                           (' "string encoding" "%s"' % self.pick(["sRGB", "linear", "gamma 2.2"]) if self.r.random() < 0.2 else ""))
            else:
                continue
            self.float_tex.append(name)
        for i in range(self.r.randrange(0, 5)):
            name = "st%d" % i
            kind = self.pick(["constant", "scale", "mix", "checkerboard", "marble", "imagemap", "bilerp", "dots"])
            if kind == "constant":
                out.append('Texture "%s" "spectrum" "constant" "rgb value" %s' % (name, self.rgb()))
            elif kind == "scale" and self.spec_tex:
                # (a constant factor is folded into an image texture at creation, textures.cpp:927-957; a textured factor is not)
                fac = '"texture scale" "%s"' % self.pick(self.float_tex) if self.float_tex and self.r.random() < 0.3 else '"float scale" [ %s ]' % f(self.pick([1.0, self.u(0.2, 1)]))
                out.append('Texture "%s" "spectrum" "scale" "texture tex" "%s" %s' % (name, self.pick(self.spec_tex), fac))
            elif kind == "mix" and self.spec_tex:
                out.append('Texture "%s" "spectrum" "mix" "texture tex1" "%s" "rgb tex2" %s %s' % (name, self.pick(self.spec_tex), self.rgb(), self.float_param("amount", 0, 1)))
            elif kind == "checkerboard":
                out.append('Texture "%s" "spectrum" "checkerboard" "rgb tex1" %s "rgb tex2" %s' % (name, self.rgb(), self.rgb()) + self.mapping())
            elif kind == "marble":
                out.append('Texture "%s" "spectrum" "marble" "float scale" [ %s ] "float variation" [ %s ]' % (name, f(self.u(0.5, 3)), f(self.u(0.1, 0.5))))
            elif kind == "imagemap":
                out.append('Texture "%s" "spectrum" "imagemap" "string filename" "%s" "string filter" "%s" "float scale" [ %s ] "bool invert" %s'
                           % (name, os.path.join(GOLDEN, self.pick(["wood.pfm", "png_rgb8.png", "png_rgba8.png", "png_rgb16.png", "png_pal8.png"])), self.pick(["bilinear", "point", "trilinear", "ewa"]), f(self.u(0.5, 1.2)), self.pick(["true", "false"])) + self.mapping())
            elif kind == "bilerp":
                out.append('Texture "%s" "spectrum" "bilerp" "rgb v00" %s "rgb v01" %s "rgb v10" %s "rgb v11" %s' % (name, self.rgb(), self.rgb(), self.rgb(), self.rgb()))
            elif kind == "dots":
                out.append('Texture "%s" "spectrum" "dots" "rgb inside" %s "rgb outside" %s' % (name, self.rgb(), self.rgb()) + self.mapping())
            else:
                continue
            self.spec_tex.append(name)
        return out

    def material(self, name):
        # ("mix" hashes heap pointers in the reference where its amount lies strictly between 0 and 1: statistical, tests/test_oracle_golden.py;
        #  its amounts here are 0 / 1 only — a constant, or a point-filtered lookup of an image of zeros and ones through a planar mapping of the
        #  hit's position, which on an animated primitive is the position at the ray's time)
        t = self.pick(["diffuse"] * 3 + ["conductor", "dielectric", "thindielectric", "diffusetransmission", "coateddiffuse", "coatedconductor", "hair", "subsurface", "measured", "interface", "mix"])
        rough = lambda pre="": ('%s "bool remaproughness" %s' % (self.float_param(pre + "roughness", 0, 0.6), self.pick(["true", "false"]))
                                if self.r.random() < 0.6 else '"float %suroughness" [ %s ] "float %svroughness" [ %s ]' % (pre, f(self.u(0, 0.5)), pre, f(self.u(0, 0.5))))
        extra = ""
        if self.r.random() < 0.15 and self.float_tex:
            extra = ' "texture displacement" "%s"' % self.pick(self.float_tex)
        if self.r.random() < 0.1:
            extra += ' "string normalmap" "%s"' % os.path.join(GOLDEN, self.pick(["normal.pfm", "png_normal.png"]))
        if t == "diffuse":
            body = self.spectrum_param("reflectance")
        elif t == "conductor":
            body = ('"spectrum eta" "%s" "spectrum k" "%s" ' % self.pick([("metal-Cu-eta", "metal-Cu-k"), ("metal-Au-eta", "metal-Au-k"), ("metal-Al-eta", "metal-Al-k")])
                    if self.r.random() < 0.5 else self.spectrum_param("reflectance", 0.3, 0.95) + " ") + rough()
        elif t == "dielectric":
            body = ('"float eta" [ %s ] ' % f(self.u(1.1, 2.2)) if self.r.random() < 0.7 else '"spectrum eta" "%s" ' % self.pick(["glass-BK7", "glass-F11", "glass-SF11"])) + rough()
        elif t == "thindielectric":
            body = '"float eta" [ %s ]' % f(self.u(1.1, 2))
        elif t == "diffusetransmission":
            body = self.spectrum_param("reflectance", 0.05, 0.6) + " " + self.spectrum_param("transmittance", 0.05, 0.6) + ' "float scale" [ %s ]' % f(self.u(0.5, 1.2))
        elif t == "coateddiffuse":
            body = self.spectrum_param("reflectance") + " " + rough() + ' "float thickness" [ %s ] "float g" [ %s ] "rgb albedo" %s "integer maxdepth" [ %d ] "integer nsamples" [ %d ]' % (
                f(self.u(0.001, 0.1)), f(self.u(-0.5, 0.7)), self.pick(["[ 0 0 0 ]", self.rgb(0, 0.8)]), self.pick([3, 10]), self.pick([1, 2]))
        elif t == "coatedconductor":
            body = rough("interface.") + " " + rough("conductor.") + ' "float thickness" [ %s ] "rgb albedo" %s "float g" [ %s ]' % (f(self.u(0.001, 0.1)), self.pick(["[ 0 0 0 ]", self.rgb(0, 0.6)]), f(self.u(-0.5, 0.7)))
            if self.r.random() < 0.5:
                body += " " + self.spectrum_param("reflectance", 0.3, 0.95)
        elif t == "hair":
            body = self.pick(['"float eumelanin" [ %s ] "float pheomelanin" [ %s ]' % (f(self.u(0, 4)), f(self.u(0, 2))), '"rgb reflectance" %s' % self.rgb(), '"rgb sigma_a" %s' % self.rgb(0.05, 2)]) + \
                ' "float beta_m" [ %s ] "float beta_n" [ %s ] "float alpha" [ %s ]' % (f(self.u(0.1, 0.9)), f(self.u(0.1, 0.9)), f(self.u(0, 4)))
        elif t == "subsurface":
            body = self.pick(['"string name" "%s"' % self.pick(["Skin1", "Marble", "Ketchup", "Apple"]), '"rgb reflectance" %s "rgb mfp" %s' % (self.rgb(0.3, 0.9), self.rgb(0.05, 0.5)),
                              '"rgb sigma_a" %s "rgb sigma_s" %s' % (self.rgb(0.001, 0.05), self.rgb(0.5, 3))]) + ' "float scale" [ %s ] "float eta" [ %s ] "float g" [ %s ] ' % (f(self.u(0.5, 20)), f(self.u(1.2, 1.6)), f(self.u(-0.3, 0.6))) + rough()
        elif t == "measured":
            body = '"string filename" "%s"' % os.path.join(GOLDEN, self.pick(["measured_iso.bsdf", "measured_aniso.bsdf"]))
        elif t == "interface":
            body = ""
            extra = ""
        else:   # mix of two earlier named materials
            prev = [m for m in self.materials if m[1] not in ("interface", "mix", "subsurface")]
            if len(prev) < 2:
                return self.material(name)
            a, b = self.r.sample(prev, 2)
            extra = ""
            if self.r.random() < 0.3:
                body = '"string materials" [ "%s" "%s" ] "float amount" [ %d ]' % (a[0], b[0], self.pick([0, 1]))
            else:
                tex = 'Texture "%s_amount" "float" "imagemap" "string filename" "%s" "string filter" "point" "string mapping" "planar" "vector3 v1" [ %s ] "vector3 v2" [ %s ]\n' % (
                    name, os.path.join(GOLDEN, "checker01.pfm"), f(self.u(-1, 1), self.u(-1, 1), self.u(-1, 1)), f(self.u(-1, 1), self.u(-1, 1), self.u(-1, 1)))
                self.materials.append((name, t))
                return tex + 'MakeNamedMaterial "%s" "string type" "mix" "string materials" [ "%s" "%s" ] "texture amount" "%s_amount"' % (name, a[0], b[0], name)
        self.materials.append((name, t))
        return 'MakeNamedMaterial "%s" "string type" "%s" %s%s' % (name, t, body, extra)

    def emit(self, name, lo, hi):
        """an emission parameter: rgb (RGBIlluminantSpectrum), a blackbody temperature, or a named illuminant (round 4, end)"""
        k = self.r.random()
        if k < 0.7:
            return '"rgb %s" %s' % (name, self.rgb(lo, hi))
        if k < 0.85:
            return '"blackbody %s" [ %s ]' % (name, f(self.u(2500, 9000)))
        return '"spectrum %s" "%s"' % (name, self.pick(["stdillum-D65", "stdillum-A", "illum-F4", "stdillum-D50"]))

    def lights(self):
        out = []
        n = self.r.randrange(1, 4)
        kinds = ["infinite", "infinite_image", "infinite_portal", "distant", "point", "spot", "goniometric", "projection"]
        for _ in range(n):
            k = self.pick(kinds)
            sc = ' "float scale" [ %s ]' % f(self.u(0.5, 2)) if self.r.random() < 0.3 else ""
            if k == "infinite":
                out.append('LightSource "infinite" "rgb L" %s' % self.rgb(0.1, 0.6) + sc + (' "float illuminance" [ %s ]' % f(self.u(1, 5)) if self.r.random() < 0.2 else ""))
            elif k == "infinite_image":
                out.append('AttributeBegin\nRotate %s 0 0 1\nLightSource "infinite" "string filename" "%s"%s\nAttributeEnd' % (f(self.u(0, 360)), os.path.join(GOLDEN, "sky.pfm"), sc))
            elif k == "infinite_portal":
                out.append('LightSource "infinite" "string filename" "%s" "point3 portal" [ -3 5 0  3 5 0  3 5 5  -3 5 5 ]' % os.path.join(GOLDEN, "sky.pfm"))
            elif k == "distant":
                out.append('LightSource "distant" "point3 from" [ %s ] "point3 to" [ 0 0 0 ] %s' % (f(self.u(-4, 4), self.u(-4, 4), self.u(3, 9)), self.emit("L", 0.5, 2)) + sc +
                           (' "float illuminance" [ %s ]' % f(self.u(1, 6)) if self.r.random() < 0.2 else ""))
            elif k == "point":
                out.append('LightSource "point" "point3 from" [ %s ] %s' % (f(self.u(-4, 4), self.u(-5, 1), self.u(2, 6)), self.emit("I", 5, 40)) + (' "float power" [ %s ]' % f(self.u(50, 400)) if self.r.random() < 0.3 else ""))
            elif k == "spot":
                out.append('LightSource "spot" "point3 from" [ %s ] "point3 to" [ %s ] "float coneangle" [ %s ] "float conedeltaangle" [ %s ] "rgb I" %s'
                           % (f(self.u(-4, 4), self.u(-5, 0), self.u(3, 6)), f(self.u(-1, 1), self.u(-1, 1), 1), f(self.u(15, 50)), f(self.u(1, 12)), self.rgb(20, 90)) +
                           (' "float power" [ %s ]' % f(self.u(50, 500)) if self.r.random() < 0.25 else ""))
            elif k == "goniometric":
                out.append('AttributeBegin\nTranslate %s\nLightSource "goniometric" "string filename" "%s" "rgb I" %s%s\nAttributeEnd' % (f(self.u(-2, 2), self.u(-3, 0), self.u(2, 5)), os.path.join(GOLDEN, "sky.pfm"), self.rgb(5, 30),
                           ' "float power" [ %s ]' % f(self.u(50, 400)) if self.r.random() < 0.25 else ""))
            else:
                out.append('AttributeBegin\nTranslate %s\nRotate 120 1 0 0\nLightSource "projection" "string filename" "%s" "float fov" [ %s ] "float scale" [ %s ]\nAttributeEnd'
                           % (f(self.u(-2, 2), self.u(-5, -2), self.u(2, 5)), os.path.join(GOLDEN, "wood.pfm"), f(self.u(30, 80)), f(self.u(20, 80))) if self.r.random() < 0.75 else
                           'AttributeBegin\nTranslate %s\nRotate 120 1 0 0\nLightSource "projection" "string filename" "%s" "float fov" [ %s ] "float power" [ %s ]\nAttributeEnd'
                           % (f(self.u(-2, 2), self.u(-5, -2), self.u(2, 5)), os.path.join(GOLDEN, "wood.pfm"), f(self.u(30, 80)), f(self.u(100, 900))))
        return out

    def shape(self):
        """one random shape around the origin of its own frame (unit-ish size)"""
        k = self.pick(["quad", "quad", "blob", "sphere", "sphere", "disk", "cylinder", "bilinear", "curve", "subdiv", "ply"])
        alpha = ""
        if self.r.random() < 0.15:
            alpha = ' "float alpha" [ %s ]' % f(self.pick([0.0, 0.4, 0.7])) if self.r.random() < 0.5 or not self.float_tex else ' "texture alpha" "%s"' % self.pick(self.float_tex)
        if k == "quad":
            uv = ' "point2 uv" [ 0 0 1 0 1 1 0 1 ]' if self.r.random() < 0.7 else ""
            nrm = ' "normal N" [ 0.1 0 1  0 0.1 1  -0.1 0 1  0 -0.1 1 ]' if self.r.random() < 0.3 else ""
            # (round 4) "S" shading tangents: random vectors, one of them sometimes zero (the dpdu fallback of shapes.h:956-957)
            tan = ""
            if self.r.random() < 0.25:
                S = [(self.u(-1, 1), self.u(-1, 1), self.u(-0.3, 0.3)) for _ in range(4)]
                if self.r.random() < 0.3:
                    S[self.r.randrange(4)] = (0.0, 0.0, 0.0)
                tan = ' "vector3 S" [ %s ]' % "  ".join(f(*v) for v in S)
            return 'Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -1 -1 0  1 -1 0  1 1 0  -1 1 0 ]' + uv + nrm + tan + alpha
        if k == "blob":
            # an octahedron with perturbed vertices
            P = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
            P = [tuple(c + self.u(-0.2, 0.2) for c in p) for p in P]
            idx = "0 2 4  2 1 4  1 3 4  3 0 4  2 0 5  1 2 5  3 1 5  0 3 5"
            return 'Shape "trianglemesh" "integer indices" [ %s ] "point3 P" [ %s ]' % (idx, " ".join(f(*p) for p in P)) + alpha
        if k == "sphere":
            s = 'Shape "sphere" "float radius" [ %s ]' % f(self.u(0.4, 1.2))
            if self.r.random() < 0.4:
                s += ' "float zmin" [ %s ] "float zmax" [ %s ] "float phimax" [ %s ]' % (f(self.u(-0.9, -0.1)), f(self.u(0.1, 0.9)), f(self.u(90, 360)))
            return s + alpha
        if k == "disk":
            return 'Shape "disk" "float radius" [ %s ] "float innerradius" [ %s ] "float height" [ %s ] "float phimax" [ %s ]' % (f(self.u(0.5, 1.3)), f(self.pick([0, self.u(0.1, 0.4)])), f(self.u(-0.3, 0.3)), f(self.pick([360, self.u(90, 350)]))) + alpha
        if k == "cylinder":
            return 'Shape "cylinder" "float radius" [ %s ] "float zmin" [ %s ] "float zmax" [ %s ] "float phimax" [ %s ]' % (f(self.u(0.3, 0.9)), f(self.u(-1, -0.2)), f(self.u(0.2, 1)), f(self.pick([360, self.u(90, 350)]))) + alpha
        if k == "bilinear":
            return 'Shape "bilinearmesh" "integer indices" [ 0 1 2 3 ] "point3 P" [ -1 -1 %s  1 -1 %s  -1 1 %s  1 1 %s ]' % (f(self.u(-.4, .4)), f(self.u(-.4, .4)), f(self.u(-.4, .4)), f(self.u(-.4, .4))) + \
                (' "point2 uv" [ 0 0 1 0 0 1 1 1 ]' if self.r.random() < 0.5 else "") + \
                (' "string emissionfilename" "%s"' % os.path.join(GOLDEN, self.pick(["sky.pfm", "wood.pfm", "alpha.pfm"])) if self.r.random() < 0.3 else "") + alpha
        if k == "curve":
            ctype = self.pick(["flat", "cylinder", "ribbon"])
            return 'Shape "curve" "string type" "%s" "point3 P" [ -1 0 0  -0.3 %s 0.5  0.4 %s -0.3  1 0 0.2 ] "float width0" [ %s ] "float width1" [ %s ]' % (
                ctype, f(self.u(-1, 1)), f(self.u(-1, 1)), f(self.u(0.05, 0.3)), f(self.u(0.02, 0.3))) + \
                (' "normal N" [ 0 0 1  0 1 1 ]' if ctype == "ribbon" or self.r.random() < 0.3 else "")   # (a ribbon without N is the reference's ErrorExit: one scene in fifteen was lost to it)
        if k == "subdiv":
            return ('Shape "loopsubdiv" "integer levels" [ %d ] "integer indices" [ 0 2 4  2 1 4  1 3 4  3 0 4  2 0 5  1 2 5  3 1 5  0 3 5 ] '
                    '"point3 P" [ 1 0 0  -1 0 0  0 1 0  0 -1 0  0 0 1  0 0 -1 ]' % self.pick([1, 2, 3]))
        return 'Shape "plymesh" "string filename" "%s"' % os.path.join(GOLDEN, self.pick(["bilinear_quads.ply", "displace_cone.ply", "ball.ply.gz"])) + \
            (' "texture displacement" "%s" "float edgelength" [ 0.5 ]' % self.pick(self.float_tex) if self.float_tex and self.r.random() < 0.3 else "")

    def placed(self, body, may_animate=False):
        if self.r.random() < 0.12:   # (round 4, end) ConcatTransform with a sheared matrix on top of the usual chain
            body = "  ConcatTransform [ 1 %s 0 0  0 1 0 0  %s 0 1 0  0 0 0 1 ]\n" % (f(self.u(-0.4, 0.4)), f(self.u(-0.3, 0.3))) + body
        # (round 5) AnimatedPrimitive: the shape / instance under an animated CTM — where this build admits it: no
        # emitter (the caller says so; the reference refuses animated area lights).  A translation, half of the time a scale too; NO rotation: the reference
        # bounds a rotating primitive through the zeros of its motion derivative (util/transform.cpp:434-960, not restated), this build
        # through samples of the path — the boxes, and with them the scene bounds the lights are preprocessed with, differ in the last
        # bits, and the comparison here is bit for bit (tests/golden/animated.pbrt has rotations under a ground plane that fixes the bounds)
        animated = may_animate and self.r.random() < 0.25
        if animated:
            anim = "  ActiveTransform EndTime\n  Translate %s\n" % f(self.u(-0.6, 0.6), self.u(-0.6, 0.6), self.u(-0.3, 0.5))
            if self.r.random() < 0.5:
                anim += "  Scale %s\n" % f(self.u(0.7, 1.4), self.u(0.7, 1.4), self.u(0.7, 1.4))
            body = anim + "  ActiveTransform All\n" + body
        return "AttributeBegin\n  Translate %s\n  Rotate %s %s\n  Scale %s\n%s\nAttributeEnd" % (
            f(self.u(-3, 3), self.u(-2.5, 2.5), self.u(0.3, 2.5)), f(self.u(0, 360)), f(self.u(-1, 1), self.u(-1, 1), self.u(0.2, 1)),
            # (the mirror never under an animated CTM: Transform::Decompose leaves the flip in R — "XXX TODO FIXME deal with flip",
            # util/transform.cpp:223 —, the quaternion of an improper R is not a unit one, hasRotation comes out true for a pure
            # translation and the reference's interpolated matrices and motion bounds are both off: seeds 1400047/50/68/73/79/89)
            f(self.u(0.4, 1.3), self.u(0.4, 1.3), self.u(0.4, 1.3)) if self.r.random() < 0.8 or animated else f(-0.8, 0.9, 1.1), body)

    def world(self):
        out = ["WorldBegin"]
        if "fog" in self.media:
            # the camera's `MediumInterface "" "fog"` stays in the graphics state: shapes would inherit an interface with an empty inside,
            # on which the reference is not deterministic (tests/golden/open_partial_medium_interface.pbrt)
            out.append('MediumInterface "fog" "fog"')
        out += self.lights()
        out += self.textures()
        if self.r.random() < 0.25:
            if self.r.random() < 0.5:
                out.append('MakeNamedMedium "cloud" "string type" "uniformgrid" "integer nx" 2 "integer ny" 2 "integer nz" 2 "float density" [ 0.2 1 0.5 0.8 1 0.1 0.6 0.9 ] '
                           '"point3 p0" [ -1 -1 -1 ] "point3 p1" [ 1 1 1 ] "rgb sigma_a" [ 0.1 0.1 0.1 ] "rgb sigma_s" [ 0.8 0.8 0.8 ] "float scale" [ %s ]' % f(self.u(0.5, 4)))
            elif self.r.random() < 0.4:
                out.append('MakeNamedMedium "cloud" "string type" "homogeneous" "string preset" "%s" "float scale" [ %s ]' % (self.pick(["Skin1", "Wholemilk", "Ketchup"]), f(self.u(0.01, 0.2))))
            else:
                # (round 4, end) the other medium types of the path: rgb grid with emission, density grid with a temperature grid, procedural cloud
                k = self.pick(["rgbgrid", "tempgrid", "cloud"])
                g = f(self.u(-0.4, 0.8))
                if k == "rgbgrid":
                    v = lambda lo, hi: " ".join(f(self.u(lo, hi)) for _ in range(24))
                    out.append('MakeNamedMedium "cloud" "string type" "rgbgrid" "integer nx" 2 "integer ny" 2 "integer nz" 2 "point3 p0" [ -1 -1 -1 ] "point3 p1" [ 1 1 1 ] '
                               '"float scale" [ %s ] "float g" [ %s ] "float Lescale" [ %s ] "rgb sigma_a" [ %s ] "rgb sigma_s" [ %s ] "rgb Le" [ %s ]'
                               % (f(self.u(0.5, 4)), g, f(self.u(0, 2)), v(0.0, 0.1), v(0.0, 0.9), v(0.0, 0.5)))
                elif k == "tempgrid":
                    out.append('MakeNamedMedium "cloud" "string type" "uniformgrid" "integer nx" 2 "integer ny" 2 "integer nz" 2 "point3 p0" [ -1 -1 -1 ] "point3 p1" [ 1 1 1 ] '
                               '"float scale" [ %s ] "float g" [ %s ] "float Lescale" [ %s ] "rgb sigma_a" [ 0.2 0.2 0.2 ] "rgb sigma_s" [ 0.9 0.9 1.1 ] '
                               '"float temperaturescale" [ %s ] "float temperatureoffset" [ %s ] "float density" [ %s ] "float temperature" [ %s ]'
                               % (f(self.u(0.5, 4)), g, f(self.u(0.2, 1.5)), f(self.u(0.8, 1.3)), f(self.u(0, 200)),
                                  " ".join(f(self.u(0, 1)) for _ in range(8)), " ".join(f(self.u(250, 1400)) for _ in range(8))))
                else:
                    out.append('MakeNamedMedium "cloud" "string type" "cloud" "float density" [ %s ] "float wispiness" [ %s ] "float frequency" [ %s ] "float g" [ %s ] '
                               '"point3 p0" [ -1 -1 -1 ] "point3 p1" [ 1 1 1 ]' % (f(self.u(0.5, 3)), f(self.u(0.5, 2)), f(self.u(2, 6)), g))
            self.media.append("cloud")
        for i in range(self.r.randrange(2, 6)):
            out.append(self.material("m%d" % i))
        # ground
        ground = [m for m in self.materials if m[1] not in ("interface", "hair")]
        out.append('NamedMaterial "%s"' % (self.pick(ground)[0] if ground else "m0"))
        out.append('Shape "trianglemesh" "integer indices" [ 0 1 2 0 2 3 ] "point3 P" [ -7 -7 0  7 -7 0  7 7 0  -7 7 0 ] "point2 uv" [ 0 0 4 0 4 4 0 4 ]')
        # an object instance definition
        have_def = self.r.random() < 0.3
        if have_def:
            solid = [m for m in self.materials if m[1] != "interface"]
            def_mat = self.pick(solid) if solid else ("m0", self.materials[0][1] if self.materials else "diffuse")
            first, second = self.shape(), self.shape()
            if NESTED_ANIMATED and self.r.random() < 0.5:
                # an animated shape inside the definition (scene.cpp:287-288): a translation, half of the time a scale too, no rotation (see placed())
                anim = "ActiveTransform EndTime\n  Translate %s\n" % f(self.u(-0.6, 0.6), self.u(-0.6, 0.6), self.u(-0.3, 0.5))
                if self.r.random() < 0.5:
                    anim += "  Scale %s\n" % f(self.u(0.7, 1.4), self.u(0.7, 1.4), self.u(0.7, 1.4))
                second = anim + "  ActiveTransform All\n  " + second
            out.append('ObjectBegin "thing"\n  NamedMaterial "%s"\n  %s\n  Translate 0 0 1.2\n  %s\nObjectEnd' % (def_mat[0], first, second))
        for i in range(self.r.randrange(2, 7)):
            name, t = self.pick(self.materials)
            body = '  NamedMaterial "%s"\n' % name
            if t == "interface":
                if not self.media:
                    continue
                body += '  MediumInterface "%s" "%s"\n' % (self.pick(self.media), "fog" if "fog" in self.media else "")
            elif self.media and t in ("dielectric", "thindielectric") and self.r.random() < 0.3:
                body += '  MediumInterface "%s" "%s"\n' % (self.pick(self.media), "fog" if "fog" in self.media else "")
            emitter = False
            if self.r.random() < 0.2 and t not in ("interface",):
                body += '  AreaLightSource "diffuse" "rgb L" %s%s\n' % (self.rgb(1, 8), ' "bool twosided" true' if self.r.random() < 0.5 else "") + \
                        (('  # image emission\n') if False else "")
                emitter = True
            if self.r.random() < 0.15:
                body += "  ReverseOrientation\n"
            body += "  " + self.shape()
            out.append(self.placed(body, may_animate=not emitter))
        if have_def:
            for _ in range(self.r.randrange(1, 4)):
                out.append(self.placed('  ObjectInstance "thing"', may_animate=True))
        if "fog" in self.media:
            # A ray that travels in a medium and MISSES every surface is pushed by MediumSampleQueue::Push(RayWorkItem, tMax), which leaves the
            # item's `depth` unwritten (wavefront/workitems.h:468-492): the reference then reads a stale depth and its image depends on
            # the threads' push order.  With the camera inside a medium the scene is therefore closed by a far sphere: no ray misses.
            solid = [m for m in self.materials if m[1] in ("diffuse", "conductor", "coateddiffuse", "diffusetransmission")]
            if solid:
                out.append('AttributeBegin\n  NamedMaterial "%s"\n  Shape "sphere" "float radius" [ 40 ]\nAttributeEnd' % self.pick(solid)[0])
            else:
                out.append('AttributeBegin\n  Material "diffuse"\n  Shape "sphere" "float radius" [ 40 ]\nAttributeEnd')
        return out

    def scene(self):
        h = self.header()
        # the camera medium must be declared in front of the camera
        if "fog" in self.media:
            i = next(k for k, l in enumerate(h) if l.startswith("Camera"))
            mk = next(k for k, l in enumerate(h) if l.startswith("MakeNamedMedium"))
            decl = h.pop(mk)
            h.insert(i, 'MediumInterface "" "fog"')
            h.insert(i, decl)
        return "\n".join(h + self.world()) + "\n"


def render(exe, args, path, out):
    try:
        p = subprocess.run([exe] + args + ["--outfile", out, path], capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        return "timeout", ""
    # "CHECK_RARE failures" (pbrt.cpp:146): the reference's CPU build counts how often a rare branch is taken (a total internal reflection
    # in a rough dielectric, ...: CHECK_RARE, util/check.h:96-112 — compiled OUT of its GPU code, :89-92) and exits with status 1 AFTER the
    # image is written when a frequency is above its threshold, which a 33 x 19 image at 4 spp reaches easily: the image is the verdict
    if p.returncode == 1 and os.path.exists(out) and "CHECK_RARE failures" in (p.stdout + p.stderr):
        return "ok", ""
    if p.returncode != 0 or not os.path.exists(out):
        return "error(%d)" % p.returncode, (p.stdout + p.stderr)[-400:]
    return "ok", ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--keep", default="/tmp/wf_diff_findings")
    ap.add_argument("--first", type=int, default=0, help="index of the first scene of the seed's sequence (re-run one scene: --first I --n 1)")
    ap.add_argument("--options", action="store_true", help="also draw the Option directives disablepixeljitter / disablewavelengthjitter / disabletexturefiltering / seed / displacementedgescale")
    ap.add_argument("--stress", action="store_true", help="rare grammar features two to three times as often (StressRandom)")
    ap.add_argument("--nested-animated", action="store_true", help="half of the object instance definitions hold a shape under an animated CTM (an AnimatedPrimitive inside the definition)")
    a = ap.parse_args()
    global STRESS, EXTENDED_OPTIONS, NESTED_ANIMATED
    STRESS = a.stress
    EXTENDED_OPTIONS = a.options
    NESTED_ANIMATED = a.nested_animated
    work = tempfile.mkdtemp(prefix="wf_diff_")
    stats = {"identical": 0, "both_refuse": 0, "mismatch": 0, "status_differs": 0}
    for i in range(a.first, a.first + a.n):
        seed = a.seed * 100000 + i
        text = Gen(seed).scene()
        path = os.path.join(work, "s%d.pbrt" % seed)
        open(path, "w").write(text)
        ro, co = os.path.join(work, "ref.pfm"), os.path.join(work, "cpu.pfm")
        for q in (ro, co):
            if os.path.exists(q):
                os.unlink(q)
        rs, rmsg = render(REF, ["--wavefront", "--quiet", "--seed", "0", "--nthreads", "4"], path, ro)
        cs, cmsg = render(CPU, ["--quiet", "--nthreads", "4"], path, co)
        verdict = None
        if rs == "ok" and cs == "ok":
            r, c = read_pfm(ro), read_pfm(co)
            if r.shape == c.shape and (r.view(np.uint32) == c.view(np.uint32)).all():
                stats["identical"] += 1
            else:
                # is the reference itself deterministic here?  (it is not on medium transitions with an empty side: see
                # tests/golden/open_partial_medium_interface.pbrt)
                ro2, ro3 = os.path.join(work, "ref2.pfm"), os.path.join(work, "ref3.pfm")
                rs2, _ = render(REF, ["--wavefront", "--quiet", "--seed", "0", "--nthreads", "2"], path, ro2)
                rs3, _ = render(REF, ["--wavefront", "--quiet", "--seed", "0", "--nthreads", "1"], path, ro3)
                if (rs2 == "ok" and not (read_pfm(ro2).view(np.uint32) == r.view(np.uint32)).all()) or (rs3 == "ok" and not (read_pfm(ro3).view(np.uint32) == r.view(np.uint32)).all()):
                    stats["reference_nondeterministic"] = stats.get("reference_nondeterministic", 0) + 1
                    print("seed %d: the reference gives two different images in two runs (no parity target)" % seed, flush=True)
                    os.unlink(path)
                    continue
                # The reference's MediumSampleQueue::Push(RayWorkItem, tMax) — the push of a ray that missed every surface — leaves the item's
                # `depth` unwritten (wavefront/workitems.h:468-492): SampleMediumInteraction reads the depth of the slot's previous user, which
                # depends on the order the threads push in.  Sequentially the port can reproduce it (wf_cpu --emulate-stale-medium-depth):
                # a difference that goes away under it is the reference's order dependence, not a parity bug.
                ro1, co1 = os.path.join(work, "ref1.pfm"), os.path.join(work, "cpu1.pfm")
                rs1, _ = render(REF, ["--wavefront", "--quiet", "--seed", "0", "--nthreads", "1"], path, ro1)
                cs1, _ = render(CPU, ["--quiet", "--emulate-stale-medium-depth"], path, co1)
                if rs1 == "ok" and cs1 == "ok" and (read_pfm(ro1).view(np.uint32) == read_pfm(co1).view(np.uint32)).all():
                    stats["reference_stale_medium_depth"] = stats.get("reference_stale_medium_depth", 0) + 1
                    print("seed %d: differs only through the reference's unwritten MediumSampleWorkItem::depth (identical under sequential emulation)" % seed, flush=True)
                    os.unlink(path)
                    continue
                # ... and the unwritten depth of a slot that NO ray has used before is whatever the heap held (the queues come from
                # plain operator new): scenes whose loading frees large blocks (PLY readers, animated shapes) hand the queue recycled
                # memory, ref_trace prints depths like 2118233313, and an UNUSED texture declaration changes the reference's image
                # (finding s1800074, round 5).  glibc's MALLOC_PERTURB_ fills every allocation with a byte pattern: a reference whose
                # image changes under it reads memory it never wrote — no parity target.  (A port bug in such a scene stays unseen.)
                uninit = False
                if rs1 == "ok":
                    base = read_pfm(ro1)
                    for pat in ("85", "170"):
                        rop = os.path.join(work, "refp.pfm")
                        if os.path.exists(rop):
                            os.unlink(rop)
                        os.environ["MALLOC_PERTURB_"] = pat
                        rsp, _ = render(REF, ["--wavefront", "--quiet", "--seed", "0", "--nthreads", "1"], path, rop)
                        del os.environ["MALLOC_PERTURB_"]
                        if rsp == "ok":
                            pert = read_pfm(rop)
                            if pert.shape != base.shape or not (pert.view(np.uint32) == base.view(np.uint32)).all():
                                uninit = True
                                break
                if uninit:
                    stats["reference_uninitialised_read"] = stats.get("reference_uninitialised_read", 0) + 1
                    print("seed %d: the reference's image changes under MALLOC_PERTURB_ (it reads memory it never wrote: no parity target)" % seed, flush=True)
                    os.unlink(path)
                    continue
                verdict = "MISMATCH"
                if r.shape == c.shape:
                    d = np.abs(r - c) / np.maximum(np.abs(r), 1e-2)
                    verdict += " max rel %.3g, %.2f %% of values differ" % (d.max(), 100 * (r.view(np.uint32) != c.view(np.uint32)).mean())
                stats["mismatch"] += 1
        elif rs == "timeout":
            # (the reference needed more than five minutes — loop subdivision of an absurd level, a lens system traced over a huge film — : no verdict)
            stats["reference_timeout"] = stats.get("reference_timeout", 0) + 1
            print("seed %d: reference timeout, port %s" % (seed, cs), flush=True)
        elif rs != "ok" and cs != "ok":
            stats["both_refuse"] += 1
            if rs.startswith("error(-") or rs == "timeout":   # the reference crashed: not a refusal; say so
                print("seed %d: reference %s, port %s" % (seed, rs, cs), flush=True)
        elif rs == "error(-11)" and cs == "ok":
            # the reference died of a SIGSEGV (not an ErrorExit, not a CHECK): nothing to match.  Known case: a ray with a NaN direction in a
            # grid medium — its DDAMajorantIterator indexes voxel INT_MIN — where this build's iterator ends (wf_media.h MajorantIter::Next)
            stats["reference_segfault"] = stats.get("reference_segfault", 0) + 1
            print("seed %d: the reference segfaults, the port renders (no parity target)" % seed, flush=True)
        else:
            verdict = "STATUS reference %s / port %s: %s" % (rs, cs, (rmsg or cmsg).strip().splitlines()[-1] if (rmsg or cmsg).strip() else "")
            stats["status_differs"] += 1
        if verdict:
            os.makedirs(a.keep, exist_ok=True)
            shutil.copy(path, os.path.join(a.keep, os.path.basename(path)))
            print("seed %d: %s" % (seed, verdict), flush=True)
        os.unlink(path)
    shutil.rmtree(work, ignore_errors=True)
    print(stats)
    sys.exit(1 if stats["mismatch"] or stats["status_differs"] else 0)


if __name__ == "__main__":
    main()
