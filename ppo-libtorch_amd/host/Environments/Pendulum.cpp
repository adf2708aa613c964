#include "Pendulum.h"

#include <cmath>
#include <random>

Pendulum::Pendulum(std::shared_ptr<ppo::Device> device, int64_t seed, int64_t env_index)
    : max_speed(8.0f), max_torque(2.0f), dt(0.05f), g(10.0f), m(1.0f), l(1.0f), low{ -1.0f, -1.0f, -8.0f }, high{ 1.0f, 1.0f, 8.0f }, episode_length(0),
      episode_reward(0.0f), m_device(std::move(device)), m_seed(seed), m_env_index(env_index) {
    if (!m_device) m_device = std::make_shared<ppo::Device>(0);
}

// The arithmetic is the library's (ppo_env_transition_f32: pendulum_step, the device function every Pendulum kernel calls), as MountainCar::step's is.
std::tuple<std::vector<float>, float, bool, bool> Pendulum::step(const std::vector<float>& action) {
    using ppo::Tensor;
    Tensor s = Tensor::from_host<float>(m_device, state, { 1, 2 });
    Tensor a = Tensor::from_host<float>(m_device, { action.empty() ? 0.0f : action[0] }, { 1, 1 });
    Tensor ns(m_device, { 1, 2 }, ppo::DType::f32), ob(m_device, { 1, 3 }, ppo::DType::f32), r(m_device, { 1 }, ppo::DType::f32), t(m_device, { 1 }, ppo::DType::i32);
    ppo::check(ppo_env_transition_f32(PPO_ENV_PENDULUM, s.data<float>(), a.data<float>(), 1, ns.data<float>(), ob.data<float>(), r.data<float>(), t.data<int32_t>(),
                                      m_device->stream()),
               m_device->util(), "Pendulum::step");
    state = ns.cpu<float>();
    m_obs = ob.cpu<float>();
    const float reward = r.item<float>();
    episode_length += 1;
    episode_reward += reward;
    return { m_obs, reward, t.item<int32_t>() != 0, false };
}

// As MountainCar::randomUniform: a deterministic function of (seed, env index, reset count) through the libstdc++ uniform mapping.
std::vector<float> Pendulum::randomUniform(float lo, float hi) {
    std::seed_seq seq{ static_cast<uint32_t>(m_seed), static_cast<uint32_t>(m_env_index), static_cast<uint32_t>(m_resets++) };
    std::mt19937 gen(seq);
    std::uniform_real_distribution<float> angle(lo, hi), speed(-1.0f, 1.0f);
    const float th = angle(gen);
    return { th, speed(gen) };
}

std::vector<float> Pendulum::reset() {
    state = randomUniform(-3.14159265358979323846f, 3.14159265358979323846f);
    m_obs = { std::cos(state[0]), std::sin(state[0]), state[1] };
    episode_length = 0;
    episode_reward = 0.0f;
    return m_obs;
}
