// The compiled table of the static chain kernels (included by fftchain.hip, which says how to add a shape).
// F<n>: the plan FftContext::sub makes for length n with radices up to 9 (theta and 2-D FFT stages); G<n>: up to 8 (ring stages).
using F8 = StaticFft<8, 8>;
using F10 = StaticFft<10, 5, 2>;
using F15 = StaticFft<15, 5, 3>;
using F16 = StaticFft<16, 8, 2>;
using F21 = StaticFft<21, 7, 3>;
using F25 = StaticFft<25, 5, 5>;
using F32 = StaticFft<32, 8, 4>;
using F42 = StaticFft<42, 7, 6>;
using F48 = StaticFft<48, 8, 6>;
using F64 = StaticFft<64, 8, 8>;
using F72 = StaticFft<72, 9, 8>;
using F90 = StaticFft<90, 9, 5, 2>;
using F96 = StaticFft<96, 8, 6, 2>;
using F112 = StaticFft<112, 7, 8, 2>;
using F120 = StaticFft<120, 5, 3, 8>;
using F126 = StaticFft<126, 9, 7, 2>;
using F135 = StaticFft<135, 9, 5, 3>;
using F144 = StaticFft<144, 9, 8, 2>;
using F150 = StaticFft<150, 5, 5, 6>;
using F160 = StaticFft<160, 5, 8, 4>;
using F168 = StaticFft<168, 7, 3, 8>;
using F200 = StaticFft<200, 5, 5, 8>;
using F216 = StaticFft<216, 9, 3, 8>;
using F225 = StaticFft<225, 9, 5, 5>;
using F252 = StaticFft<252, 9, 7, 4>;
using F256 = StaticFft<256, 8, 8, 4>;
using F270 = StaticFft<270, 9, 5, 6>;
using F300 = StaticFft<300, 5, 5, 6, 2>;
using F336 = StaticFft<336, 7, 8, 6>;
using G3 = StaticFft<3, 3>;
using G8 = F8;
using G40 = StaticFft<40, 5, 8>;
using G45 = StaticFft<45, 5, 3, 3>;
using G75 = StaticFft<75, 5, 5, 3>;
using G80 = StaticFft<80, 5, 8, 2>;
using G90 = StaticFft<90, 5, 3, 6>;
using G135 = StaticFft<135, 5, 3, 3, 3>;
using G180 = StaticFft<180, 5, 6, 6>;
using G240 = StaticFft<240, 5, 8, 6>;
using G256 = F256;
using G288 = StaticFft<288, 8, 6, 6>;
using G320 = StaticFft<320, 5, 8, 8>;
static const std::vector<StaticEntry>& static_table() {
	static const std::vector<StaticEntry> t = {
		PXS_CS(StFirst, F8, NoFft, 136)
		PXS_CS(StFirst, F8, NoFft, 256)
		// over its stage's register budget, left to the run-time kernel: StFirst, F48, T = 48 (68 VGPRs against the stage's 67)
		PXS_CS(StFirst, F64, NoFft, 16)
		PXS_CS(StFirst, F64, NoFft, 32)
		PXS_CS(StFirst, F72, NoFft, 32)
		PXS_CS(StFirst, F96, NoFft, 24)
		PXS_CS(StFirst, F160, NoFft, 16)
		PXS_CS(StResize, F16, F32, 64)
		PXS_CS(StResize, F25, F42, 56)
		PXS_CS(StResize, F32, F16, 64)
		PXS_CS(StResize, F32, F32, 64)
		PXS_CS(StResize, F42, F21, 56)
		PXS_CS(StResize, F112, F150, 16)
		PXS_CS(StResize, F126, F270, 8)
		PXS_CS(StResize, F135, F256, 8)
		PXS_CS(StResize, F168, F300, 8)
		PXS_CS(StResize, F225, F252, 8)
		PXS_CS(StResize, F225, F336, 7)
		PXS_CS(StResize, F252, F126, 8)
		PXS_CS(StResize, F256, F270, 8)
		PXS_CS(StResize, F270, F135, 8)
		PXS_CS(StResize, F270, F252, 8)
		PXS_CS(StResize, F336, F168, 7)
		PXS_CS(StSigma, F8, F8, 272)
		PXS_CS(StSigma, F48, F48, 48)
		PXS_CS(StSigma, F64, F64, 32)
		PXS_CS(StSigma, F72, F72, 32)
		PXS_CS(StSigma, F96, F96, 24)
		PXS_CS(StSigma, F160, F160, 16)
		PXS_CS(StSplit<0>, F8, NoFft, 272)
		PXS_CS(StSplit<0>, F48, NoFft, 48)
		PXS_CS(StSplit<0>, F64, NoFft, 32)
		PXS_CS(StSplit<0>, F72, NoFft, 32)
		PXS_CS(StSplit<0>, F96, NoFft, 24)
		PXS_CS(StSplit<0>, F160, NoFft, 16)
		PXS_CS(StSplit<1>, F8, NoFft, 320)
		PXS_CS(StSplit<1>, F64, NoFft, 40)
		PXS_CS(StSplit<1>, F72, NoFft, 32)
		// over its stage's register budget, left to the run-time kernel: StSplit<1>, F160, T = 16 (79 VGPRs against the stage's 71)
		PXS_CS(StRingA1, G3, NoFft, 80)
		PXS_CS(StRingA1, G8, NoFft, 256)
		PXS_CS(StRingA1, G40, NoFft, 48)
		PXS_CS(StRingA1, G45, NoFft, 48)
		PXS_CS(StRingA1, G90, NoFft, 16)
		PXS_CS(StRingA1, G180, NoFft, 16)
		PXS_CS(StRingA2, G45, NoFft, 56)
		PXS_CS(StRingA2, G80, NoFft, 32)
		PXS_CS(StRingA2, G240, NoFft, 8)
		PXS_CS(StRingA2, G256, NoFft, 8)
		PXS_CS(StRingS1, G45, NoFft, 40)
		PXS_CS(StRingS1, G240, NoFft, 8)
		PXS_CS(StRingS1, G256, NoFft, 8)
		PXS_CS(StRingS1, G288, NoFft, 8)
		PXS_CS(StRingS1, G320, NoFft, 8)
		PXS_CS(StRingS2, G8, NoFft, 256)
		PXS_CS(StRingS2, G40, NoFft, 48)
		PXS_CS(StRingS2, G45, NoFft, 48)
		PXS_CS(StRingS2, G75, NoFft, 32)
		PXS_CS(StRingS2, G135, NoFft, 16)
		PXS_CS(StColOut, F15, NoFft, 128)
		PXS_CS(StColOut, F15, NoFft, 168)
		PXS_CS(StColOut, F16, NoFft, 152)
		PXS_CS(StColOut, F120, NoFft, 16)
		PXS_CS(StColOut, F150, NoFft, 16)
		PXS_CS(StColOut, F216, NoFft, 8)
		PXS_CS(StFirst2D, F10, NoFft, 16)
		PXS_CS(StFirst2D, F15, NoFft, 16)
		// over its stage's register budget, left to the run-time kernel: StFirst2D, F90, T = 24 (68 VGPRs against the stage's 66)
		PXS_CS(StFirst2D, F144, NoFft, 16)
		PXS_CS(StFirst2D, F200, NoFft, 8)
	};
	return t;
}
