#include "Acrobot.h"

#include <cmath>
#include <random>

namespace {
const float PI_F = 3.14159265358979323846f, TWO_PI_F = 6.28318530717958647692f, HALF_PI_F = 1.57079632679489661923f;
const float MAX_W1 = 12.566370614359172f, MAX_W2 = 28.274333882308138f, DT6 = static_cast<float>(0.2 / 6.0);
const double TWO_PI_D = 6.283185307179586476925;

// |x| >= 64: reduced in binary64, every operation rounded on its own, then rounded to f32 (ppo_hip.h: PPO_ENV_ACROBOT, "the trigonometric range")
float reduce(float x) {
    if (std::fabs(x) < 64.0f) return x;
    const double xd = static_cast<double>(x);
    const double q = std::rint(xd / TWO_PI_D);
    const double p = TWO_PI_D * q;
    return static_cast<float>(xd - p);
}

void dsdt(const float* s, float tau, float* k) {
    const float th1 = s[0], th2 = s[1], w1 = s[2], w2 = s[3];
    const float c2 = Acrobot::cosr(th2), s2 = Acrobot::sinr(th2);
    const float d1 = (0.25f + (1.25f + c2)) + 2.0f;
    const float d2 = (0.25f + 0.5f * c2) + 1.0f;
    const float phi2 = 4.9f * Acrobot::cosr((th1 + th2) - HALF_PI_F);
    const float phi1 = (((-0.5f * (w2 * w2)) * s2 - (w2 * w1) * s2) + 14.7f * Acrobot::cosr(th1 - HALF_PI_F)) + phi2;
    const float dw2 = (((tau + (d2 / d1) * phi1) - (0.5f * (w1 * w1)) * s2) - phi2) / (1.25f - (d2 * d2) / d1);
    const float dw1 = -(d2 * dw2 + phi1) / d1;
    k[0] = w1; k[1] = w2; k[2] = dw1; k[3] = dw2;
}

float wrap(float x) {
    for (int i = 0; i < 1024 && x > PI_F; i++) x -= TWO_PI_F;
    for (int i = 0; i < 1024 && x < -PI_F; i++) x += TWO_PI_F;
    return x;
}
}  // namespace

float Acrobot::sinr(float x) { return std::sin(reduce(x)); }
float Acrobot::cosr(float x) { return std::cos(reduce(x)); }

float Acrobot::transition(float* st, int action, bool& terminated) {
    const float tau = static_cast<float>(action) - 1.0f;
    float k1[4], k2[4], k3[4], k4[4], y[4];
    dsdt(st, tau, k1);
    for (int i = 0; i < 4; i++) y[i] = st[i] + 0.1f * k1[i];
    dsdt(y, tau, k2);
    for (int i = 0; i < 4; i++) y[i] = st[i] + 0.1f * k2[i];
    dsdt(y, tau, k3);
    for (int i = 0; i < 4; i++) y[i] = st[i] + 0.2f * k3[i];
    dsdt(y, tau, k4);
    for (int i = 0; i < 4; i++) y[i] = st[i] + DT6 * (((k1[i] + 2.0f * k2[i]) + 2.0f * k3[i]) + k4[i]);
    const float th1 = wrap(y[0]), th2 = wrap(y[1]);
    const float w1 = y[2] < -MAX_W1 ? -MAX_W1 : (y[2] > MAX_W1 ? MAX_W1 : y[2]);
    const float w2 = y[3] < -MAX_W2 ? -MAX_W2 : (y[3] > MAX_W2 ? MAX_W2 : y[3]);
    st[0] = th1; st[1] = th2; st[2] = w1; st[3] = w2;
    terminated = (-cosr(th1)) - cosr(th2 + th1) > 1.0f;
    return terminated ? 0.0f : -1.0f;
}

void Acrobot::observe(const float* st, float* obs) {
    obs[0] = cosr(st[0]);
    obs[1] = sinr(st[0]);
    obs[2] = cosr(st[1]);
    obs[3] = sinr(st[1]);
    obs[4] = st[2];
    obs[5] = st[3];
}

Acrobot::Acrobot(int64_t seed, int64_t env_index) : state(4, 0.0f), episode_length(0), episode_reward(0.0f), m_seed(seed), m_env_index(env_index) {}

std::vector<float> Acrobot::observation() const {
    std::vector<float> obs(6);
    observe(state.data(), obs.data());
    return obs;
}

std::tuple<std::vector<float>, float, bool, bool> Acrobot::step(int64_t action) {
    bool terminated = false;
    const float reward = transition(state.data(), static_cast<int>(action), terminated);
    episode_length += 1;
    episode_reward += reward;
    return { observation(), reward, terminated, false };
}

// As MountainCar::randomUniform: a deterministic function of (seed, env index, reset count) through the libstdc++ uniform mapping
std::vector<float> Acrobot::reset() {
    std::seed_seq seq{ static_cast<uint32_t>(m_seed), static_cast<uint32_t>(m_env_index), static_cast<uint32_t>(m_resets++) };
    std::mt19937 gen(seq);
    std::uniform_real_distribution<float> dis(-0.1f, 0.1f);
    for (float& v : state) v = dis(gen);
    episode_length = 0;
    episode_reward = 0.0f;
    return observation();
}
